/*
 * include/gdr.h — C ABI of libgdr_hip.so, the MI355X (gfx950) differentiable
 * Gaussian-splatting rasterizer for the Generative Densification render path.
 *
 * This is the drop-in boundary: the entry points below are what a binding of the
 * reference's rasterizer extension would call.  The reference reaches its CUDA
 * extension through the Python package `diff_gaussian_rasterization`
 *   - import:            /root/reference/lightning/renderer.py:10-13
 *                        /root/reference/lightning/point_decoder/layers/gaussian_renderer.py:14
 *   - settings record:   /root/reference/lightning/renderer.py:111-124 (12 fields)
 *   - forward call:      /root/reference/lightning/renderer.py:250-259
 *                        (-> color(3,H,W), radii(N), depth(1,H,W), alpha(1,H,W))
 *   - backward contract: /root/reference/lightning/network.py:867-878
 *                        ((N,4) means2D gradient, |.|-accumulated in columns 2-3)
 * whose native half (`_C.rasterize_gaussians`, `_C.rasterize_gaussians_backward`,
 * `_C.mark_visible`; un-vendored submodule, /root/reference/.gitmodules:1-3) is what
 * these functions replace.  See INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / HIP types in any signature
 *     (`stream` is a hipStream_t passed as void*; NULL = the null stream);
 *   - every pointer is a DEVICE pointer to fp32/int32 data unless it says "host";
 *   - matrices are 16 contiguous floats in the reference's row-vector convention
 *     (/root/reference/lightning/utils.py:37-47): p_view = [p,1] @ viewmatrix;
 *   - the caller owns every buffer; the library allocates no device memory.  Process-wide state it DOES keep (all
 *     mutex-guarded; results never depend on any of it except where said): (1) the per-shape view history behind
 *     gdr_view_plan_for — duplicates per Gaussian and launch-size reports of recent calls, gdr_view_history_*;
 *     (2) the K7 choice per launch shape, gdr_k7_tune_* — decided per shape by timing (once + one confirmation), so WHICH of two
 *     kernels sums a gradient (the same terms in another order: differences at the fp32 rounding level) can differ
 *     between processes unless gdr_k7_tune_override pins it; (3) pooled pinned words / events (gdr_host_copy_*,
 *     gdr_forward_view(s), gdr_view_reuse_probe); (4) the opt-in timing facility at the end of this header.
 *     Re-entrant, thread-safe for distinct workspaces, one call per stream;
 *   - all work is enqueued on `stream`; the only host synchronisation is the
 *     optional read-back of num_rendered in gdr_preprocess_forward;
 *   - return value: 0 = GDR_OK, negative = error (never throws across the ABI).
 */
#ifndef GDR_H
#define GDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDR_ABI_VERSION 17

#define GDR_OK 0
#define GDR_ERR_INVALID_ARG (-1)  /* NULL / inconsistent arguments                     */
#define GDR_ERR_HIP (-2)          /* a HIP call failed: see gdr_last_error()           */
#define GDR_ERR_UNSUPPORTED (-3)  /* sh_degree > 3, image too large for the key layout */
#define GDR_ERR_WORKSPACE (-4)    /* caller workspace smaller than required            */

/* The storage type of a buffer's elements, wherever an entry point takes a `dtype`.  Each module's own names below
 * (GDR_ATTN_*, GDR_SUBM_*, GDR_SEG_*, GDR_NORM_*) are these; which of them an entry point accepts is stated with it. */
#define GDR_F16 0
#define GDR_BF16 1
#define GDR_F32 2

/* Size limits of this build (checked at every entry point, GDR_ERR_UNSUPPORTED beyond them):
 * per-Gaussian element offsets are computed in 32-bit registers up to 9*N (SH rows use 64-bit
 * offsets), and num_rendered is a 32-bit counter as in the reference's int num_rendered. */
#define GDR_MAX_GAUSSIANS (1 << 27) /* 134 M Gaussians: 32 GB of degree-3 inputs               */
#define GDR_MAX_RENDERED 0xFFFFFFFFull /* D = sum of tiles_touched of one view                  */

#define GDR_DEFAULT_DEEP_MAX_BUSY 768 /* gdr_binning.deep_max_busy as carved: 3/4 of the 1024 resident K6 workgroups */
#define GDR_DEFAULT_SEG_LEN 256 /* gdr_binning.seg_len as carved (the library reads no environment variable); callers may
                                 * raise it after carving.  2048 in round 1; short segments balance K7's (tile, segment)
                                 * workgroups: 512 vs 2048 C3 shell 2130 -> 2640, C2 shell 1970 -> 2460 views/s at the same
                                 * speed on uniform scenes; 256 gains another 4-6 % on 512x512 images and loses 2 % at
                                 * 2 M Gaussians 800x800, so the Python host raises it to 512 for >= 2000 tiles. */
#define GDR_TILE 16 /* tile edge in pixels (BLOCK_X = BLOCK_Y = 16) */

/* The 12 fields of GaussianRasterizationSettings (renderer.py:111-124), flattened.
 * bg / viewmatrix / projmatrix / campos stay device tensors exactly as the caller
 * holds them (no host copies, no sync). */
typedef struct gdr_settings {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    float scale_modifier;
    int32_t sh_degree;   /* active degree, 0..3 */
    int32_t prefiltered; /* accepted, unused (reference always passes False) */
    int32_t debug;       /* !=0: synchronise + check after every kernel */
    const float* bg;         /* (3)  */
    const float* viewmatrix; /* (16) */
    const float* projmatrix; /* (16) */
    const float* campos;     /* (3)  */
} gdr_settings;

/* Per-Gaussian inputs of GaussianRasterizer.forward (renderer.py:250-259).
 * Exactly one of shs / colors_precomp and one of (scales, rotations) / cov3D_precomp
 * is non-NULL. */
typedef struct gdr_inputs {
    int32_t N;                   /* number of Gaussians */
    int32_t M;                   /* SH coefficients per Gaussian stored in `shs` (>= (deg+1)^2) */
    const float* means3D;        /* (N,3) */
    const float* opacities;      /* (N)   activated, [0,1] */
    const float* shs;            /* (N,M,3) or NULL */
    const float* colors_precomp; /* (N,3)   or NULL */
    const float* scales;         /* (N,3)   or NULL, activated */
    const float* rotations;      /* (N,4)   or NULL, (r,x,y,z), used as given */
    const float* cov3D_precomp;  /* (N,6)   or NULL */
    uint32_t flags;              /* GDR_IN_RAW_*: fold the adaptor's activations into K1/K9 */
    uint32_t reserved;
} gdr_inputs;

/* gdr_inputs.flags — the render adaptor (lightning/renderer.py:225-230) applies sigmoid to the
 * opacity logits, exp to the log-scales and F.normalize to the quaternions before calling the
 * rasterizer.  With a flag set the corresponding pointer holds the RAW tensor, the activation
 * runs inside K1 and its derivative inside K9 (the returned gradient is w.r.t. the raw tensor). */
#define GDR_IN_RAW_OPACITY 1u
#define GDR_IN_RAW_SCALES 2u
#define GDR_IN_RAW_ROTATIONS 4u
/* parity-risk switch R1: the CUDA fork's source is unavailable, so whether its backward sends
 * dL/d(depth image) into the Gaussian centres (depth_i = z of the centre in view space) is unknown; default = it
 * does (ashawkey lineage).  With this flag the depth gradient still reaches the opacities / conics / 2D means
 * through the blend weights, but no longer moves the centres along the view axis. */
#define GDR_IN_NO_DEPTH_TO_MEAN 8u

/* Geometry state written by the forward and re-read by the backward
 * (upstream "geomBuffer").  Carved from one caller allocation by gdr_geom_carve. */
typedef struct gdr_geom {
    float* depths;           /* (N)   camera-space z                         */
    float* rec;              /* (N,16) render record, ONE 64-byte line per Gaussian so that
                              * K6/K7 gather one line instead of three:
                              *   [0..1] pixel-space mean xy   [2] depth   [3] -
                              *   [4..6] inverse 2D cov (xx,xy,yy)         [7] opacity
                              *   [8..10] colour rgb            [11] depth
                              *   [12..13] half-extent of {alpha >= 1/255} (px; < 0: never)  */
    float* cov3D;            /* (N,6)                                        */
    int32_t* rect;           /* (N,4) tile rect minx,miny,maxx,maxy          */
    uint32_t* tiles_touched; /* (N)                                          */
    uint8_t* clamped;        /* (N)   bit ch set <=> colour channel clamped  */
    uint32_t* block_sums;    /* (ceil(N/256)+1) per-block sums of tiles_touched (global-sort path) */
    uint32_t* block_offs;    /* (ceil(N/256))   per-block duplicate offsets drawn from num_rendered
                              * with one atomic per block (emission order is free: the default
                              * sort orders ties by Gaussian id explicitly)                     */
    uint32_t* num_rendered;  /* (1)   D = sum tiles_touched                  */
} gdr_geom;

/* Binning state (upstream "binningBuffer"): D (key,value) pairs, double-buffered. */
typedef struct gdr_binning {
    uint64_t* keys[2];   /* (D) each.  Direct tile binning (default): keys[0] holds ONE packed word per entry of the partitioned
                          * list, id << 32 | float_bits(depth), which the per-tile depth sort consumes; keys[1] is unused.  Radix
                          * partition / global sort: the (tile << 32) | float_bits(depth) keys, double-buffered.  The sorted
                          * 64-bit keys of the reference are never materialised on the default path (the parity tests rebuild
                          * them from ranges + sorted ids + depths) */
    uint32_t* values[2]; /* (D) Gaussian index                              */
    uint32_t* hist;      /* radix-sort scratch                              */
    int32_t sorted;      /* which of the two buffers holds the sorted list  */
    int32_t global_sort; /* !=0: one global LSD radix sort over all key bits instead of the default
                          * tile partition + per-tile LDS depth sort (same result; A/B and tests) */
    uint32_t* scratch32; /* (2*D) depth-key ping-pong for tile lists that do not fit in LDS */
    /* Segments of long tile lists (K7 walks the segments of one tile in parallel workgroups):
     * a tile whose sorted list is longer than seg_len entries is cut every seg_len entries;
     * K6 saves the per-pixel compositing state at every cut and at the end of the list. */
    uint32_t* seg_extra; /* (seg_cap,2) (tile, segment) of every segment but the last of its tile */
    uint32_t* seg_count; /* (4) rows of seg_extra, state slots, "deep forward" flag (few busy tiles), - */
    float* seg_state;    /* (2*seg_cap, 10, 256) K6 -> K7: per pixel of the tile, in front of each cut and at
                          * the end of the list: T, colour x3, depth, alpha sums (gdr); T, colour x3,
                          * normal x3, depth, M1, M2 (gsr)                                          */
    int32_t seg_len;     /* entries per segment (multiple of 256); 0 = lists are never cut.  gdr_binning_carve sets
                          * GDR_DEFAULT_SEG_LEN and sizes the tables for it; a caller may RAISE it or set 0 afterwards */
    int32_t seg_cap;     /* D / seg_len + 1                                                         */
    int32_t deep_max_busy; /* K6 renders the CUT tiles with 16 instead of 64 pixels per wave ("deep" forward, 4 workgroups
                          * per tile) when at most this many tiles hold >= 64 entries AND their lists average >= 2560
                          * entries — an object in front of an empty background leaves most CUs with one workgroup
                          * walking a long list.  gdr_binning_carve sets GDR_DEFAULT_DEEP_MAX_BUSY; 0 = never. */
    int32_t deep_min_mean; /* ... and their lists average at least this many entries; <= 0 = the library default (2560) */
    const uint32_t* d_dev; /* NULL (gdr_binning_carve): the D passed to the binning entry points is the duplicate count,
                          * read back from geom->num_rendered by the caller.  Non-NULL = a DEVICE-SIZED call: the binning
                          * kernels read the count from this device word (geom->num_rendered) themselves and the D passed
                          * to gdr_binning_carve / gdr_binning_forward* is only the CAPACITY the buffers were carved for —
                          * the caller can enqueue binning + K6 behind K1 without waiting for K1, and compares the count
                          * with the capacity afterwards.  A count above the capacity is clamped (nothing is written out
                          * of bounds; the images are then incomplete and the view must be repeated with enough room). */
    /* Launch-size feedback between calls that render the same kind of scene (all optional, results never depend on it):
     * the binning stage reports what it found, the caller passes it back into the next call of that shape. */
    uint32_t* stats_out; /* NULL, or 4 device-writable words (pinned host memory works): {tiles in the tile sort's long
                          * class (> 4096 entries), tiles in its medium class (2049..4096), "deep forward" flag, busy tiles} */
    int32_t hint_long;   /* > 0: workgroups for the tile sort's long class; 0 = sized for the worst case; < 0: the long class
                          * (16 waves, 144 KB of LDS per workgroup) is not launched, the medium class takes any longer list
                          * through its global-memory bucket pass (same result, slower for such a list).  Every value >= 1 */
    int32_t hint_medium; /*      is correct (the classes walk their tiles with a grid stride), a wrong one only costs time   */
    int32_t hint_no_deep;/* != 0: the deep forward is not launched; K6 renders every tile the standard way (same images)     */
    int32_t grad_rec_cleared; /* != 0: the caller has already zero-filled the gradient record it passes to the K7 entry points
                          * for this view (e.g. early, on a side stream, while the forward still runs): they skip their own
                          * clear of N*64 bytes */
    uint32_t* tile_hist; /* direct tile binning (gdr_binning_carve_for): the (hist_width rows x hist_tiles columns) count matrix of
                          * the counting sort on the tile id + one row of tile totals; NULL (gdr_binning_carve, or an image
                          * of more than 16384 tiles): the radix partition on the tile bits is used instead (same lists) */
    int32_t hist_width;  /* rows of tile_hist = workgroups of the count / scatter kernels, <= 256 */
    int32_t hist_tiles;  /* columns of tile_hist = the tile count it was carved for, rounded up to 64; a binning call on an image
                          * with more tiles than that uses the radix partition instead (same lists) — was reserved1 until v14 */
    int32_t k7_class;    /* v16: duplicates per Gaussian of the view as a quarter-octave class (1..63), set by gdr_forward_view(s)
                          * from the exact count; 0 = unknown.  Part of the key under which the library remembers which K7
                          * serves a scene (gdr_k7_tune_*) — nothing else reads it */
    int32_t scatter_mode;/* how tile_scatter writes the partitioned lists (same lists up to the order within a tile, which the per-tile
                          * sort removes): 0 = the library's choice (gdr_set_scatter_mode), 1 = direct, one store per entry
                          * straight into the list, 2 = staged in LDS and written out in runs wherever a workgroup's entries
                          * fit the staging buffer; + 4: count-matrix row = workgroup index instead of the XCD-contiguous
                          * map (measurement).  The carve functions set 0.  (The field was named reserved2.) */
} gdr_binning;

/* Image state (upstream "imgBuffer"). */
typedef struct gdr_image {
    uint32_t* ranges;    /* (tiles,2) [first,last) into the sorted list     */
    uint32_t* n_contrib; /* (H*W) 1-based index of the last contributor     */
    float* final_T;      /* (H*W) transmittance after the last contributor  */
    uint32_t* tile_order; /* (tiles) tile ids, longest sorted list first (launch order of K6/K7) */
    uint32_t* seg_base;   /* (tiles) first seg_state slot of a tile whose list is cut, 0xFFFFFFFF otherwise */
} gdr_image;

typedef struct gdr_outputs {
    float* color;   /* (3,H,W) */
    float* depth;   /* (1,H,W) sum_i w_i z_i (not normalised) */
    float* alpha;   /* (1,H,W) sum_i w_i = 1 - T_final        */
    int32_t* radii; /* (N)     0 = culled                     */
} gdr_outputs;

typedef struct gdr_grad_inputs {
    const float* dL_dcolor; /* (3,H,W) */
    const float* dL_ddepth; /* (H,W) or NULL (= zeros) */
    const float* dL_dalpha; /* (H,W) or NULL (= zeros) */
} gdr_grad_inputs;

/* Gradient outputs; every buffer is fully written (zeros for culled Gaussians), the
 * caller does not need to clear anything.  dL_dmeans2D is (N,4): columns 0-1 the signed
 * NDC-space gradient, columns 2-3 the sum over pixels of its absolute per-pixel terms
 * (network.py:876-878).  scratch: (N*16) floats — one 64-byte gradient record per Gaussian
 * that K7 accumulates into (mean2D, conic, depth, colour, opacity partials). */
typedef struct gdr_grad_outputs {
    float* dL_dmeans3D;   /* (N,3) */
    float* dL_dmeans2D;   /* (N,4) */
    float* dL_dshs;       /* (N,M,3) or NULL when colors_precomp was used */
    float* dL_dcolors;    /* (N,3)  or NULL when shs was used (then taken from scratch) */
    float* dL_dopacities; /* (N)   */
    float* dL_dscales;    /* (N,3) or NULL when cov3D_precomp was used */
    float* dL_drotations; /* (N,4) or NULL when cov3D_precomp was used */
    float* dL_dcov3D;     /* (N,6) or NULL when scales/rotations were used */
    float* scratch;       /* (N*16) floats, 64-byte aligned, contents undefined on return */
    int32_t accumulate;   /* !=0: ADD into the output buffers (sum over views of one Gaussian
                           * set, network.py:826-838) instead of overwriting them */
    int32_t reserved;
} gdr_grad_outputs;

/* ---- sizes and carving ---------------------------------------------------------- */
int gdr_abi_version(void);
const char* gdr_last_error(void); /* thread-local, host string */
/* "release" for the product build.  Anything else marks a measurement / experimental build of the library (compiled with
 * -DGDR_BUILD_TAG=...): the Python loader refuses to load such a library unless GDR_ALLOW_EXPERIMENTAL_LIB=1 is set. */
const char* gdr_build_tag(void);
/* Process-wide tile_scatter mode for every gdr_binning whose scatter_mode is 0 (the entry points that carve their own
 * workspace: gdr_forward_view(s), gsr_forward_view): the values of gdr_binning.scatter_mode; 0 = automatic.  Returns the
 * previous value. */
int32_t gdr_set_scatter_mode(int32_t mode);
/* Process-wide mode of the per-tile depth sort for lists of up to 4096 entries (longer lists are not affected): 0 = automatic
 * (= 2), 1 = stable 8-bit radix passes + tie pass, 2 = one counting pass on 4096 depth buckets + in-bucket fix-up, radix for
 * a list that puts more than 16 entries into one bucket.  Same sorted lists under every mode.  Returns the previous value. */
int32_t gdr_set_tile_sort_mode(int32_t mode);
/* Debug only: waits for the current device, then returns how many lists left the bucket path for the radix code since the
 * counter was last cleared (reset != 0 clears it); < 0 on a HIP error.  Results never depend on the counter. */
int64_t gdr_debug_tile_sort_fallbacks(int32_t reset);

size_t gdr_geom_bytes(int32_t N);
size_t gdr_binning_bytes(uint64_t D);
size_t gdr_image_bytes(int32_t H, int32_t W);
/* base must be 256-byte aligned and at least gdr_*_bytes(...) long. */
int gdr_geom_carve(void* base, int32_t N, gdr_geom* out);
int gdr_binning_carve(void* base, uint64_t D, gdr_binning* out);
/* The same for a known scene shape: the cut-list tables (seg_extra, seg_state: 2 * (D / seg_len + 1) slots of 10 KB —
 * 80 bytes per duplicate at seg_len = 256, 40 at 512) sized for the segment length the caller is going to use (seg_len =
 * a multiple of 256, or 0: lists are never cut, no tables; out->seg_len = seg_len), and — given N Gaussians and the
 * image's tile count — the count matrix of the direct tile binning (min(256, N / 1024) + 1 rows of tiles words; tiles = 0 or
 * > 16384: none, the radix partition is used). */
size_t gdr_binning_bytes_for(uint64_t D, int32_t seg_len, int32_t N, int32_t tiles);
int gdr_binning_carve_for(void* base, uint64_t D, int32_t seg_len, int32_t N, int32_t tiles, gdr_binning* out);
int gdr_image_carve(void* base, int32_t H, int32_t W, gdr_image* out);

/* ---- forward ---------------------------------------------------------------------
 * gdr_preprocess_forward + gdr_render_forward (or gdr_forward = both) replace the forward half of the extension,
 * `_C.rasterize_gaussians`, reached from `rasterizer(means3D=…, …)` at /root/reference/lightning/renderer.py:250-259 and
 * /root/reference/lightning/point_decoder/layers/gaussian_renderer.py:88-108.
 * Stage 1 (K1 + K2): per-Gaussian projection, EWA covariance, SH colour, tile rect,
 * and the scan total.  radii is written here.  If num_rendered_host != NULL the
 * stream is synchronised and D is returned through it (the one host read the
 * upstream extension also performs); otherwise D stays in geom->num_rendered. */
int gdr_preprocess_forward(const gdr_settings* s, const gdr_inputs* in, const gdr_geom* geom,
                           int32_t* radii, uint32_t* num_rendered_host, void* stream);

/* Stage 2 (K3..K6): duplicate with keys, radix sort on (tile, depth), tile ranges,
 * per-tile alpha-composited render.  D is the capacity of `bin` and must be >= the
 * value stage 1 produced.  bin->sorted is set. */
int gdr_render_forward(const gdr_settings* s, const gdr_inputs* in, const gdr_geom* geom,
                       gdr_binning* bin, const gdr_image* img, uint64_t D,
                       const gdr_outputs* out, void* stream);

/* The two halves of stage 2, for callers that overlap the binning of one view with the compositing of another on
 * separate streams (binning is latency-bound with few workgroups, compositing is VALU-bound):
 * gdr_binning_forward = K3..K5 + tile order + tile sort (also valid for the surfel geometry of gsr.h),
 * gdr_composite_forward = K6.  gdr_render_forward is exactly one after the other on one stream.
 * The binning stage builds the cut-list tables of `bin` (seg_extra, seg_count, img->seg_base); K6 fills seg_state
 * and every backward entry point below reads the seg_state of the LATEST compositing call on that (bin, img) pair. */
int gdr_binning_forward(const gdr_settings* s, int32_t N, const gdr_geom* geom, gdr_binning* bin, const gdr_image* img,
                        uint64_t D, const int32_t* radii, void* stream);
int gdr_composite_forward(const gdr_settings* s, const gdr_geom* geom, const gdr_binning* bin, const gdr_image* img,
                          const gdr_outputs* out, void* stream);

/* K6 / K7 with the image loss folded in ("clamp + MSE + per-view loss reduction folded into the K6/K7
 * epilogue/prologue"; renderer.py:261 clamp, loss.py:37-38 MSE, plus the depth / alpha means of the measurement loss):
 *   *loss += mean_{c,p}(clamp(color,0,1) - target)^2 + w_depth mean(depth) + w_alpha mean(alpha)
 * gdr_composite_forward_loss = K6 that also accumulates the view's loss (one atomic per tile; the caller zeroes *loss);
 * the images are still written.  gdr_render_backward_loss = K7 whose per-pixel upstream gradients are computed from
 * `color` (what K6 wrote) and `target` times the upstream scalar *g (device) instead of being read — no loss kernels,
 * no dL/dimage tensors.  target, color: (3,H,W). */
int gdr_composite_forward_loss(const gdr_settings* s, const gdr_geom* geom, const gdr_binning* bin, const gdr_image* img,
                               const gdr_outputs* out, const float* target, float w_depth, float w_alpha, float* loss,
                               void* stream);
int gdr_render_backward_loss(const gdr_settings* s, int32_t N, const gdr_geom* geom, const gdr_binning* bin,
                             const gdr_image* img, const float* color, const float* target, float w_depth, float w_alpha,
                             const float* g, float* grad_rec, void* stream);

/* K6 of V <= GDR_MAX_VIEWS views of one image size in ONE launch (v14; SURVEY section 7 step 5 "grid.z = view"): the
 * workgroups of all views in one grid (interleave != 0: the same launch-order slot of consecutive views next to each other).
 * Every view must have finished its binning stage on `stream`'s dependencies.  loss_mode 0 = gdr_composite_forward,
 * 1 = gdr_composite_forward_loss (losses[v] accumulated: the caller zeroes the V floats), 2 = gdr_composite_forward_lossgrad
 * (outs[v].color receives d loss / d colour, depth / alpha are not written and may be NULL). */
int gdr_composite_forward_views(int32_t V, const gdr_settings* s, const gdr_geom* geoms, const gdr_binning* bins,
                                const gdr_image* imgs, const gdr_outputs* outs, int32_t loss_mode,
                                const float* const* targets, float w_depth, float w_alpha, float go_scale, float* losses,
                                int32_t interleave, void* stream);

/* Stages 1+2 with a caller-provided binning capacity D_cap.  Synchronises once to
 * read D; returns GDR_ERR_WORKSPACE (and *num_rendered_host = required D) if
 * D > D_cap, in which case only stage 1 has run. */
int gdr_forward(const gdr_settings* s, const gdr_inputs* in, const gdr_geom* geom,
                gdr_binning* bin, const gdr_image* img, uint64_t D_cap, const gdr_outputs* out,
                uint32_t* num_rendered_host, void* stream);

/* ---- one forward call per view (v14) ------------------------------------------------------------------------------
 * The reference's extension does its whole forward in ONE native call (`_C.rasterize_gaussians`, reached from
 * /root/reference/lightning/renderer.py:250-259 inside the per-view loops of network.py:827-838).  gdr_forward_view is
 * that call: it carves ONE caller allocation into the geometry / image / binning state, runs K1, starts the duplicate
 * count on its way to pinned host memory, enqueues binning + K6 sized by the device counter, waits for the count and
 * compares it with the capacity — everything the Python boundary did with ~20 ABI calls until round 3.
 *   gdr_view_plan_for   sizes the allocation: capacity = exact_D if given, else 1.5 x the largest recent duplicate count
 *                       per Gaussian of this scene shape (device, power-of-two bucket of N, H, W) x N + 4096 — the library
 *                       keeps that small per-shape history (process-wide, mutex-guarded; gdr_view_history_reset clears it)
 *                       together with the launch-size feedback of gdr_binning.stats_out / hint_*.  No history yet:
 *                       plan.have_binning = 0 — the forward then stops behind K1 with GDR_ERR_WORKSPACE and state.D set;
 *   gdr_forward_view    returns GDR_OK with `state` filled (the structs every backward entry point takes, and D), or
 *                       GDR_ERR_WORKSPACE with state.D = the count: plan again with exact_D = state.D, allocate, call again
 *                       (the first call of a shape, or a scene that grew past the slack: nothing was written out of bounds).
 * opts (NULL = defaults): test / A-B overrides, each -1 / 0 = the library's policy.  same (NULL = none): up to 8 buffer
 * pairs compared bit for bit next to K1 (see gdr_words_differ; state.differ != 0 if any differs) — the equality check of a
 * render group rides on the count's copy.  Thread-safe for distinct workspaces. */
typedef struct gdr_view_plan {
    uint64_t capacity;     /* duplicates the binning state is carved for */
    uint64_t bytes;        /* size of the one allocation (256-byte aligned base) */
    int32_t seg_len;       /* gdr_binning.seg_len of the carve */
    int32_t deferred;      /* != 0: capacity is a guess -> device-sized call */
    int32_t have_binning;  /* 0: no history and no exact_D: geometry + image state only */
    int32_t reserved;
} gdr_view_plan;
typedef struct gdr_view_opts {
    int32_t seg_len;         /* >= 0: segment length of cut lists (0 = never cut); -1: policy (256; 512 on busy 800x800 images) */
    int32_t deep_max_busy;   /* >= 0: gdr_binning.deep_max_busy; -1: default */
    int32_t deep_min_mean;   /* >= 0: gdr_binning.deep_min_mean; -1: default */
    int32_t global_sort;     /* != 0: one global radix sort (tested fallback) */
    int32_t radix_partition; /* != 0: radix partition on the tile bits instead of the direct tile binning (tested fallback) */
    int32_t no_hints;        /* != 0: no launch-size feedback */
} gdr_view_opts;
#define GDR_SAME_AS_MAX 8
typedef struct gdr_same_as {
    int32_t n;               /* <= GDR_SAME_AS_MAX (4 until v15; a caller that re-activates all five inputs per call has 5 pairs) */
    int32_t reserved;
    const void* a[GDR_SAME_AS_MAX]; const void* b[GDR_SAME_AS_MAX]; uint64_t n_bytes[GDR_SAME_AS_MAX];
} gdr_same_as;
typedef struct gdr_view_state {
    gdr_geom geom; gdr_binning bin; gdr_image img;
    uint64_t D;              /* duplicates of the view (the reference's num_rendered) */
    uint32_t differ;         /* != 0: a same-as pair differed */
    uint32_t reserved;
} gdr_view_state;
int gdr_view_plan_for(int32_t N, int32_t H, int32_t W, int32_t surfel, uint64_t exact_D, const gdr_view_opts* opts,
                      gdr_view_plan* plan);
int gdr_forward_view(const gdr_settings* s, const gdr_inputs* in, const gdr_view_plan* plan, void* workspace,
                     const gdr_view_opts* opts, const gdr_same_as* same, const gdr_outputs* out, gdr_view_state* state,
                     void* stream);
/* Does the view about to be rendered repeat an earlier view of the same Gaussians (v16)?  The reference renders the first
 * n_views_sel views of the coarse Gaussians twice per sample — /root/reference/lightning/network.py:827-838, then again inside
 * the function `vjp` differentiates at :848-856, with the same c2w / bg_color — and a render group (viewgroup.py) that knows
 * the Gaussians are the same only has to know that the 12 settings fields are, too, to hand out the first forward's results
 * instead of running K1, binning and K6 again.  The host scalars of `s` are compared here on the host; bg / viewmatrix /
 * projmatrix / campos (device tensors the caller rebuilds per call: MiniCam at network.py:851) are compared bit for bit on
 * the device against up to GDR_REUSE_MAX candidates in one small launch, together with the `same` pairs of the render group
 * (gdr_same_as: the activated tensors of this call against the group's).  BLOCKING: *match = index of the first candidate
 * whose 12 fields equal those of `s` (or -1), *differ != 0 if a `same` pair differs — one launch, one pooled pinned copy,
 * one event wait.  scratch: GDR_REUSE_MAX + 1 device words (the library allocates no device memory). */
#define GDR_REUSE_MAX 32
int gdr_view_reuse_probe(const gdr_settings* s, int32_t n, const gdr_settings* candidates, const gdr_same_as* same,
                         uint32_t* scratch, int32_t* match, uint32_t* differ, void* stream);

/* The same for ALL views of one Gaussian set (the forward of the multi-view node, v14): V <= GDR_MAX_NODE_VIEWS views of one
 * image size; K1 in launches of <= GDR_MAX_VIEWS views (inputs read once each), then every view's chain binning -> K6 on
 * streams[v % n_streams] (streams[0] = the caller's: it is made to wait for the others before the call returns), the V
 * duplicate counts read back with ONE pooled pinned copy after everything is enqueued.  ONE allocation for all views
 * (gdr_views_plan_for: V x the per-view state + the packed counters).  loss_mode / targets / w_* / go_scale / losses as in
 * gdr_composite_forward_views.  states: V structs, filled (cov3D of every view points at view 0's copy).  Returns GDR_OK, or
 * GDR_ERR_WORKSPACE with every states[v].D set: plan again with exact_D = the largest of them and call again. */
#define GDR_MAX_NODE_VIEWS 256
typedef struct gdr_views_plan {
    gdr_view_plan view;      /* the per-view plan (capacity, seg_len, deferred, have_binning) */
    uint64_t bytes_view;     /* stride between the views' state in the allocation */
    uint64_t bytes_shared;
    uint64_t bytes;          /* V x bytes_view + bytes_shared */
    int32_t V;
    int32_t reserved;
} gdr_views_plan;
int gdr_views_plan_for(int32_t V, int32_t N, int32_t H, int32_t W, uint64_t exact_D, const gdr_view_opts* opts,
                       gdr_views_plan* plan);
int gdr_forward_views(int32_t V, const gdr_settings* s, const gdr_inputs* in, const gdr_views_plan* plan, void* workspace,
                      const gdr_view_opts* opts, const gdr_outputs* outs, int32_t loss_mode, const float* const* targets,
                      float w_depth, float w_alpha, float go_scale, float* losses, void* const* streams, int32_t n_streams,
                      gdr_view_state* states);
void gdr_view_history_reset(void);
/* the history behind gdr_view_plan_for, per scene shape: the decaying maximum of duplicates per Gaussian (0 = none yet).
 * _set seeds or overrides it — a caller that knows its scene statistics skips the read-back of a shape's first call; the
 * tests force an overflow with a tiny value (the call then answers GDR_ERR_WORKSPACE and is repeated exactly sized). */
/* the launch-size report words of a shape's previous call (row = view of the call, < 64): {tiles in the tile sort's long class,
 * in its medium class, "deep forward applied", busy tiles}, 0xFFFFFFFF = nothing reported yet; set != 0 overwrites them (tests:
 * wrong hints must only cost time) */
int gdr_view_history_report(int32_t N, int32_t H, int32_t W, int32_t surfel, int32_t row, uint32_t* words, int32_t set);
double gdr_view_history_get(int32_t N, int32_t H, int32_t W, int32_t surfel);
void gdr_view_history_set(int32_t N, int32_t H, int32_t W, int32_t surfel, double duplicates_per_gaussian);
/* Which K7 serves a scene shape (v15).  K7 publishes one float-atomic record line per (list entry, 4x4 pixel block) hit and
 * the device retires ~21 G such lines per second whatever they carry: wherever Gaussians span several blocks that rate, not
 * the arithmetic, bounds K7.  A second kernel lets the two rows of an 8x4 area walk the union of their lists and publish
 * ONE line where that saves enough lines per extra iteration — faster for Gaussians of 10+ pixels spread over the image,
 * slower for sub-pixel Gaussians and object-like scenes.  The gradients are the same sums in another order.  Per (device,
 * N bucket, duplicates-per-Gaussian class of the views — gdr_binning.k7_class —, image size, views per launch, entry kind)
 * the library times both kernels ONCE (events around four consecutive launches, rows / pairs / rows / pairs, after the key's
 * first 8 launches; never on a stream under graph capture) and keeps the faster (v16; until v15 the round was repeated every
 * 256 launches, so the variant could change mid-run).  v17: ONE confirmation — launches 64..67 of the key time both kernels
 * once more and the first pick is overturned only if it loses that round by > 5 % (a wrong pick from one noisy timing cost
 * 3 % at C4, 15 % at C2 for the life of the process); after it the choice is final.  A scene that drifts moves to another
 * class, i.e. another key with rounds of its own.
 * kind: 0 gdr_backward / gdr_render_backward(_views), 1 the _loss entries, 2 the mean2D-only entries, 3 the 2DGS K7s
 * (gsr_backward / gsr_render_backward(_views): 16 + 4 totals per pair, two record lines), 4 gdr_render_backward_mean2d_loss.
 * _override: -1 measure and choose (default), 0 rows only, 1 row pairs always (tests, A/B, bit-reproducible runs: the Python
 * loader maps GDR_K7_PAIRS=0/1 onto it).  _get: the choice (-1 = not decided yet: rows serve meanwhile) and the round's times in
 * microseconds of the most recently used key of that (N bucket, image size, V, kind) — error if there is none.
 * gdr_view_history_reset restarts the choices. */
void gdr_k7_tune_override(int32_t mode);
int gdr_k7_tune_get(int32_t N, int32_t H, int32_t W, int32_t V, int32_t kind, int32_t* chosen, float* us_rows, float* us_pairs);
/* v17: both rounds of that key — *rounds_done 0 (first round still to come / running), 1 (decided once), 2 (confirmed: final);
 * us4 = {rows, pairs} of the first round, {rows, pairs} of the confirmation round, microseconds, 0 = not measured yet. */
int gdr_k7_tune_get_rounds(int32_t N, int32_t H, int32_t W, int32_t V, int32_t kind, int32_t* chosen, int32_t* rounds_done,
                           float* us4);
/* test hook: make `variant` the FIRST pick of that key (as if its first round had chosen it) — the confirmation round must
 * then correct it if it is the wrong one.  Error once the key's choice is final. */
int gdr_k7_tune_force_first(int32_t N, int32_t H, int32_t W, int32_t V, int32_t kind, int32_t variant);

/* ---- backward (K7 + K8/K9) --------------------------------------------------------
 * Replaces `_C.rasterize_gaussians_backward`, reached through autograd from the losses on the render outputs
 * (/root/reference/lightning/network.py:746-752, 836, 854, 971) and through `vjp` w.r.t. the (N,4) means2D carrier
 * (/root/reference/lightning/network.py:865-878). */
int gdr_backward(const gdr_settings* s, const gdr_inputs* in, const gdr_geom* geom,
                 const gdr_binning* bin, const gdr_image* img, uint64_t D,
                 const int32_t* radii, const gdr_grad_inputs* gin, const gdr_grad_outputs* gout,
                 void* stream);

/* ---- multi-view entry points (one Gaussian set, V <= GDR_MAX_VIEWS views of one image size) ----
 * The callers render all target views of one Gaussian set back to back
 * (/root/reference/lightning/network.py:826-838, 848-856, 964-972).  These variants do the
 * view-independent work once: the per-Gaussian inputs are read once for all V views, cov3D is
 * written once (to geoms[0].cov3D — every geoms[v].cov3D is ignored), and the backward sums the
 * V per-view partial gradients in registers before writing each output once.
 * s, geoms: arrays of V structs; radii, grad_recs: arrays of V device pointers (host arrays).
 * Requires in->shs, in->scales, in->rotations (no colors_precomp / cov3D_precomp).
 * Sequence: gdr_preprocess_forward_views; read the V values geoms[v].num_rendered (or, for
 *           device-sized calls — gdr_binning.d_dev — only start copying them to the host);
 *           per view gdr_render_forward; (device-sized: compare counts and capacities, repeat
 *           the views that did not fit); ...; per view gdr_render_backward (K7 into its own
 *           N*16-float record); gdr_preprocess_backward_views. */
#define GDR_MAX_VIEWS 8
int gdr_preprocess_forward_views(int32_t V, const gdr_settings* s, const gdr_inputs* in,
                                 const gdr_geom* geoms, int32_t* const* radii, void* stream);
int gdr_render_backward(const gdr_settings* s, int32_t N, const gdr_geom* geom, const gdr_binning* bin,
                        const gdr_image* img, const gdr_grad_inputs* gin, float* grad_rec,
                        void* stream);
int gdr_preprocess_backward_views(int32_t V, const gdr_settings* s, const gdr_inputs* in,
                                  const gdr_geom* geoms, const int32_t* const* radii,
                                  float* const* grad_recs, const gdr_grad_outputs* gout, void* stream);

/* K7 of V <= GDR_MAX_VIEWS views of one image size in ONE launch (v14).  The views of a node are independent given the
 * Gaussians; one launch over V x (segments + tiles) workgroups keeps the chip full across the views' kernel tails where V
 * launches on side streams leave it to the dispatcher (reference-scale scenes: one view is 1-2.5 k workgroups for 1280
 * resident slots).  Arrays of V structs / V device pointers (host arrays); every view writes its own N*16-float record
 * (cleared here unless bins[v].grad_rec_cleared).  interleave != 0: consecutive workgroups take the same slot of
 * consecutive views (all views' longest work items first); 0: the views follow one another in the grid (a view's
 * records — 128 MB at 2 M Gaussians — are not evicted from the caches by the other views' gathers).
 * _loss_views: g = device array of V upstream scalars (see gdr_render_backward_loss); colors / targets: V x (3,H,W).
 * _mean2d_views: every view ADDS into the one (N,4) buffer (see gdr_render_backward_mean2d). */
int gdr_render_backward_views(int32_t V, const gdr_settings* s, int32_t N, const gdr_geom* geoms, const gdr_binning* bins,
                              const gdr_image* imgs, const gdr_grad_inputs* gins, float* const* grad_recs,
                              int32_t interleave, void* stream);
int gdr_render_backward_loss_views(int32_t V, const gdr_settings* s, int32_t N, const gdr_geom* geoms,
                                   const gdr_binning* bins, const gdr_image* imgs, const float* const* colors,
                                   const float* const* targets, float w_depth, float w_alpha, const float* g,
                                   float* const* grad_recs, int32_t interleave, void* stream);
int gdr_render_backward_mean2d_views(int32_t V, const gdr_settings* s, int32_t N, const gdr_geom* geoms,
                                     const gdr_binning* bins, const gdr_image* imgs, const float* const* dL_dcolors,
                                     float* dL_dmean2D, int32_t interleave, void* stream);

/* ---- screen-space gradient only ----------------------------------------------
 * The densification step differentiates an image loss w.r.t. the (N,4) means2D carrier of several
 * views and uses nothing else (/root/reference/lightning/network.py:865-878).  This K7 variant
 * ADDS one view's dL/dmean2D (x, y signed; |x|, |y| summed per pixel) into dL_dmean2D (N,4), which the
 * caller zeroes once before the first view; no per-view records, no K8/K9. */
int gdr_render_backward_mean2d(const gdr_settings* s, int32_t N, const gdr_geom* geom,
                               const gdr_binning* bin, const gdr_image* img, const float* dL_dcolor,
                               float* dL_dmean2D, void* stream);

/* the same with the image MSE folded into the prologue (see gdr_render_backward_loss): the per-pixel upstream gradient
 * is *g * 2/(3 H W) * (clamp(color) - target) inside [0,1], 0 outside; no dL/dimage tensor */
int gdr_render_backward_mean2d_loss(const gdr_settings* s, int32_t N, const gdr_geom* geom, const gdr_binning* bin,
                                    const gdr_image* img, const float* color, const float* target, const float* g,
                                    float* dL_dmean2D, void* stream);

/* The abs-grad-only path end to end (replaces the vjp of /root/reference/lightning/network.py:843-878 and the
 * torch.topk of :876-893):
 *   gdr_composite_forward_lossgrad   K6 with the MSE of one view folded in and NO image output: loss += mean_{c,p}
 *                                    (clamp(color) - target)^2 (device float, caller zeroes), and dL_dcolor (3,H,W) :=
 *                                    go_scale * d loss / d color per pixel — the only per-pixel array it writes besides the
 *                                    backward state (final T, contributor count).  go_scale = the upstream scalar known on
 *                                    the host (1 / views for a mean over the views).
 *   gdr_render_backward_mean2d       consumes that dL_dcolor (above).
 *   gdr_topk_absgrad                 selection on score_i = ||dL_dmean2D[i, 2:4]||_2: mask[i] = 1 for the k largest
 *                                    scores among the candidates (candidates == NULL: all N; fewer than k candidates —
 *                                    counted on the device — : every candidate with score >= 0, the reference's
 *                                    `gradient_point >= 0` branch, which drops NaN; otherwise NaN ranks above every
 *                                    number, as in torch.topk); indices (k, may be
 *                                    NULL) receives the selected ids in no particular order (the reference only builds
 *                                    a mask from them).  Radix select, no sort; ties at the threshold are cut arbitrarily,
 *                                    as torch.topk leaves them.  workspace: gdr_topk_workspace_bytes() bytes. */
int gdr_composite_forward_lossgrad(const gdr_settings* s, const gdr_geom* geom, const gdr_binning* bin, const gdr_image* img,
                                   const float* target, float go_scale, float* loss, float* dL_dcolor, void* stream);
size_t gdr_topk_workspace_bytes(void);
int gdr_topk_absgrad(int32_t N, const float* dL_dmean2D, const uint8_t* candidates, int32_t k, void* workspace,
                     uint8_t* mask, int32_t* indices, void* stream);

/* ---- fused image loss either side of the path ---------------------------------
 * loss += mean_{c,p}(clamp(color,0,1) - target)^2 + w_depth mean(depth) + w_alpha mean(alpha) for ONE view
 * (renderer.py:261 clamp, loss.py:37-38 MSE; depth/alpha terms: the measurement loss of SURVEY §8d).
 * color, target: (3,H,W); depth, alpha: (H,W); loss: device float the caller zeroes (accumulated with one
 * atomic per workgroup).  backward: g = device pointer to the upstream scalar (NULL = 1). */
int gdr_view_loss_forward(const float* color, const float* depth, const float* alpha, const float* target,
                          int32_t H, int32_t W, float w_depth, float w_alpha, float* loss, void* stream);
int gdr_view_loss_backward(const float* color, const float* target, int32_t H, int32_t W, float w_depth,
                           float w_alpha, const float* g, float* dL_dcolor, float* dL_ddepth, float* dL_dalpha,
                           void* stream);

/* ---- SSIM / MS-SSIM (csrc/ssim.hip; added in v17, backward-compatible) -------------------------------------------------
 * The image-similarity half of the reference's training loss MSE + 0.5 (1 - MS-SSIM) (lightning/loss.py) and the SSIM of
 * its evaluation, with the semantics of pytorch_msssim 1.x (restated in the header of csrc/ssim.hip).  X, Y: (B, C, H, W)
 * fp32 read through element strides (b, c, h, w) — a permuted NHWC view is read in place.  out: B*C device floats, the
 * per-(batch, channel) value (ssim, relu(ssim) or the MS-SSIM product).  win: the normalised 1-D window (win_size odd,
 * <= GDR_SSIM_MAX_WIN); weights: one per level (GDR_SSIM_MS).  C1 = (K1 data_range)^2, C2 = (K2 data_range)^2.
 * workspace (gdr_ssim_workspace_bytes, 256-byte aligned) is written by forward and read by backward of the same arguments
 * (pooled pyramid, per-block partial sums, per-level coefficients).  backward: grad_out = B*C device floats (d loss / d out);
 * dX (and dY unless NULL) written through their own strides; scratch: gdr_ssim_scratch_bytes(a, dY != NULL).  No host
 * synchronisation; sizes of 0 from the _bytes queries mean the arguments are refused (gdr_last_error after the call). */
#define GDR_SSIM_MAX_WIN 15
#define GDR_SSIM_MAX_LEVELS 8
#define GDR_SSIM_PLAIN 0    /* ssim, levels = 1 */
#define GDR_SSIM_NONNEG 1   /* relu(ssim), levels = 1 */
#define GDR_SSIM_MS 2       /* ms_ssim, levels = 1..GDR_SSIM_MAX_LEVELS */
typedef struct gdr_ssim_args {
    int32_t B, C, H, W;
    int32_t win_size, levels, mode, reserved;
    float C1, C2;
    float win[GDR_SSIM_MAX_WIN];
    float weights[GDR_SSIM_MAX_LEVELS];
} gdr_ssim_args;
size_t gdr_ssim_workspace_bytes(const gdr_ssim_args* a);
size_t gdr_ssim_scratch_bytes(const gdr_ssim_args* a, int32_t want_dy);
int gdr_ssim_forward(const gdr_ssim_args* a, const float* X, const int64_t* x_strides, const float* Y,
                     const int64_t* y_strides, void* workspace, float* out, void* stream);
int gdr_ssim_backward(const gdr_ssim_args* a, const float* X, const int64_t* x_strides, const float* Y,
                      const int64_t* y_strides, const void* workspace, const float* grad_out, float* dX,
                      const int64_t* dx_strides, float* dY, const int64_t* dy_strides, void* scratch, void* stream);

/* ---- TSDF fusion and marching-cubes mesh extraction (csrc/tsdf.hip; added in v17, backward-compatible) ------------------
 * The GPU path of the reference's mesh extraction (Open3D ScalableTSDFVolume semantics, restated in the header of
 * csrc/tsdf.hip).  Views are staged one by one (gdr_tsdf_stage: sanitised f32 depth and packed 0x00BBGGRR colour, H x W
 * each; the caller stacks V of them into (V, H, W) arrays), then fused and extracted in phases whose outputs size the next
 * phase's buffers (the caller reads back: the 6-int bbox; cell_scan[cells] = n_blocks; vcount[n] and tcount[n] = the vertex
 * and triangle totals, n = n_blocks * GDR_TSDF_R^3):
 *   gdr_tsdf_bounds     bbox = {min bx, by, bz, max bx, by, bz} of the blocks touched by the sampled pixels of all views
 *   gdr_tsdf_allocate   (lo, dims = the block grid, set in args) per-cell view masks (cells * words), cell_block = the
 *                       allocated block's index in (bz, by, bx) order or -1; cell_scan: cells + 1 uint32
 *   gdr_tsdf_integrate  (n_blocks set) blocks = n_blocks x int4 (bx, by, bz, cell); vol = 5 planes of n_blocks * R^3 fp32
 *                       (tsdf, weight, r, g, b)
 *   gdr_tsdf_mc_count   cube_case (int16), vflags (uint8), vcount / tcount (n + 1 uint32) -> exclusive offsets and totals
 *   gdr_tsdf_mc_emit    vertices / colors (V x 3 fp32), triangles (F x 3 int32) in the canonical order
 *   gdr_tsdf_clusters   keys / tri_of: the 3F edge keys min(a,b) * V + max(a,b) of the triangles, sorted (stable), and the
 *                       triangle of each; label (F) = cluster rank (clusters numbered by their smallest triangle), counts
 *                       (F, first root_rank[F] used); parent (F), root_rank (F + 1) are scratch
 * scratch: gdr_tsdf_scan_bytes(the largest scanned length: cells, n or F).  Every launch on the caller's stream; nothing here
 * synchronises with the host. */
#define GDR_TSDF_R 16
typedef struct gdr_tsdf_view {
    float fx, fy, cx, cy;
    float E[12];      /* world-to-camera, rows 0..2 of the 4x4 extrinsic (f32) */
    float c2w[12];    /* camera-to-world: rows 0..2 of inverse(E) computed in f64, cast to f32 */
} gdr_tsdf_view;
typedef struct gdr_tsdf_args {
    int32_t V, H, W, stride;     /* views, image size, depth sampling stride of the allocation */
    int32_t words, n_blocks;     /* words = ceil(V / 32); n_blocks from gdr_tsdf_allocate */
    float voxel, trunc;          /* voxel length, sdf truncation */
    int32_t lo[3], dims[3];      /* block grid origin and extent (from the bbox) */
} gdr_tsdf_args;
size_t gdr_tsdf_scan_bytes(int64_t n);
int gdr_tsdf_stage(int32_t H, int32_t W, const float* depth, const int64_t* depth_strides, const void* rgb,
                   const int64_t* rgb_strides, int32_t rgb_u8, float depth_trunc, float* depth_out, uint32_t* rgb_out,
                   void* stream);
int gdr_tsdf_bounds(const gdr_tsdf_args* a, const gdr_tsdf_view* views, const float* depth, int32_t* bbox, void* stream);
int gdr_tsdf_allocate(const gdr_tsdf_args* a, const gdr_tsdf_view* views, const float* depth, uint32_t* cell_mask,
                      int32_t* cell_block, uint32_t* cell_scan, void* scratch, void* stream);
int gdr_tsdf_integrate(const gdr_tsdf_args* a, const gdr_tsdf_view* views, const float* depth, const uint32_t* rgb,
                       const uint32_t* cell_mask, const int32_t* cell_block, int32_t* blocks, float* vol, void* stream);
int gdr_tsdf_mc_count(const gdr_tsdf_args* a, const int32_t* cell_block, const int32_t* blocks, const float* vol,
                      int16_t* cube_case, uint8_t* vflags, uint32_t* vcount, uint32_t* tcount, void* scratch, void* stream);
int gdr_tsdf_mc_emit(const gdr_tsdf_args* a, const int32_t* cell_block, const int32_t* blocks, const float* vol,
                     const int16_t* cube_case, const uint8_t* vflags, const uint32_t* voff, const uint32_t* toff,
                     float* vertices, float* colors, int32_t* triangles, void* stream);
int gdr_tsdf_clusters(int32_t F, const int64_t* keys, const int64_t* tri_of, int32_t* parent, uint32_t* root_rank,
                      int32_t* label, int32_t* counts, void* scratch, void* stream);

/* ---- variable-length packed-QKV attention for short sequences (csrc/attn.hip; added in v17, backward-compatible) -------
 * The one flash_attn entry point of the reference's point decoder (flash_attn_varlen_qkvpacked_func, dropout 0, no mask):
 * per sequence b = rows [cu_seqlens[b], cu_seqlens[b + 1]) and head h, O = softmax(scale Q K^T) V over the key axis.
 * qkv: (total, 3, H, D) fp16 or bf16 read through element strides (token, q/k/v, head, channel) — a slice of a wider buffer
 * is read in place; cu_seqlens: batch + 1 device int32, or NULL: sequence b = rows [b * fixed_len, (b + 1) * fixed_len).
 * out: (total, H, D) dense in the input dtype, 16-byte aligned; lse: (H, total) dense f32 (gdr_attn_lse_bytes), the
 * per-row log-sum-exp of the scaled scores, written by forward and read by backward.  backward: dout (total, H, D) through
 * its element strides, dqkv (total, 3, H, D) dense, 16-byte aligned.  Scores, softmax and every accumulation are f32.
 * Rows at or beyond cu_seqlens[batch] (fixed_len * batch) are ZERO in out, lse and dqkv.  Envelope: D in {8, 16, 32, 64},
 * H >= 1, 1 <= max_seqlen <= GDR_ATTN_MAX_SEQLEN, any 0 <= length <= max_seqlen mixed in one call; anything else is refused
 * before any launch.  cu_seqlens is never read by the host: boundaries are clamped to [0, total] on the device and a
 * sequence longer than max_seqlen is cut (its further rows are not written).  One launch each, no atomics: two runs are
 * bitwise equal.  No host synchronisation. */
#define GDR_ATTN_MAX_SEQLEN 256
#define GDR_ATTN_F16 GDR_F16
#define GDR_ATTN_BF16 GDR_BF16
typedef struct gdr_attn_args {
    int32_t total, batch, H, D;
    int32_t max_seqlen, fixed_len;   /* fixed_len: used only when cu_seqlens == NULL */
    int32_t dtype, reserved;         /* GDR_ATTN_F16 / GDR_ATTN_BF16 */
    float scale, reserved2;          /* softmax scale (the caller resolves the default D^-0.5) */
} gdr_attn_args;
size_t gdr_attn_lse_bytes(const gdr_attn_args* a);   /* 0: the arguments are refused (gdr_last_error) */
int gdr_attn_forward(const gdr_attn_args* a, const void* qkv, const int64_t* qkv_strides, const int32_t* cu_seqlens,
                     void* out, float* lse, void* stream);
int gdr_attn_backward(const gdr_attn_args* a, const void* dout, const int64_t* dout_strides, const void* qkv,
                      const int64_t* qkv_strides, const int32_t* cu_seqlens, const void* out, const float* lse, void* dqkv,
                      void* stream);

/* ---- the same attention read and written through the decoder's index tables (csrc/attn.hip; added in v17, backward-compatible)
 * What SerializedAttention.forward of the reference runs around the call above, inside the same two kernels:
 *   out = attn(qkv[order].half().reshape(-1, 3, H, D), cu_seqlens).reshape(-1, C).to(qkv.dtype)[inverse],   C = H D
 * and that line's autograd.  qkv: (N, 3 C) dense from a 16-byte aligned base, `dtype` GDR_ATTN_F16 / BF16 / F32; every
 * element is rounded to fp16 as .half() rounds it and the arithmetic is the fp16 path of gdr_attn_forward.  order: (Tp)
 * int64, the point each padded slot holds; inverse: (N) int64, the slot that is each point's own; cu_seqlens: batch + 1
 * int32 boundaries over the Tp slots.  out: (N, C) dense in qkv's dtype: slot p stores the fp16 result, converted, to row
 * order[p] if inverse[order[p]] == p.  out_full: NULL, or (N, C) f32 that receives the same rows before any rounding.
 * lse: NULL (nothing is kept for a backward; the copy slots then compute nothing), or (H, Tp) f32 per slot.
 * backward: dout (N, C) dense in qkv's dtype (rounded to fp16 on load); out: (N, C) dense of `out_dtype`, read as it is for
 * delta_i = sum_d dO_id O_id: the forward's out (with f16 qkv that is bitwise the backward of gdr_attn_backward on the gathered
 * rows) or its out_full (a delta free of the result's rounding: for f32 and bf16 qkv); dqkv: (N, 3 C) dense in qkv's dtype.  The own slot of a row stores dQ, dK and dV, each row exactly once with plain
 * stores: two calls are bitwise equal.  A row's copy one sequence later, at the same position (the reference's padding),
 * has dQ = 0 and contributes to dK and dV: the workgroup of the own slot runs the key sweep over that next sequence too and
 * adds in f32 before the one rounding (to fp16, then to qkv's dtype).
 * Precondition for defined VALUES: order[inverse[i]] == i for every i, and every slot that is not its row's own sits one
 * sequence behind it at the same position.  Memory safety needs no precondition: no table is read by the host, entries of
 * order / inverse outside [0, N) / [0, Tp) are skipped and cu_seqlens is clamped to [0, Tp].
 * Envelope: D in {8, 16, 32, 64}, H >= 1, 1 <= max_seqlen <= GDR_ATTN_MAX_SEQLEN, N and Tp >= 0; N == 0 or Tp == 0 is a
 * no-op.  One launch each, no atomics, no scratch, no host synchronisation. */
#define GDR_ATTN_F32 GDR_F32     /* the gather entry points only */
typedef struct gdr_attn_gather_args {
    int32_t N, Tp, batch, H, D;
    int32_t max_seqlen;              /* the patch size: no sequence is longer */
    int32_t dtype, reserved;         /* GDR_ATTN_F16 / GDR_ATTN_BF16 / GDR_ATTN_F32: qkv, out, dout and dqkv */
    float scale, reserved2;          /* softmax scale (the caller resolves the default D^-0.5) */
} gdr_attn_gather_args;
int gdr_attn_gather_forward(const gdr_attn_gather_args* a, const void* qkv, const int64_t* order, const int64_t* inverse,
                            const int32_t* cu_seqlens, void* out, float* out_full, float* lse, void* stream);
int gdr_attn_gather_backward(const gdr_attn_gather_args* a, const void* dout, const void* qkv, const int64_t* order,
                             const int64_t* inverse, const int32_t* cu_seqlens, const void* out, int32_t out_dtype,
                             const float* lse, void* dqkv, void* stream);

/* ---- tiled MFMA attention for fixed-length batches of long sequences (csrc/attn_tiled.hip; added in v17, backward-compatible)
 * What a ViT image encoder runs per layer (timm Attention.forward, 1025 tokens at head dimension 64): per image b and head h,
 * O = softmax(scale Q K^T) V over the key axis, lse_i = log sum_j exp(scale Q_i . K_j).  q, k, v: (B, L, H, D) fp16 or bf16,
 * each through its own four element strides (batch, token, head, channel); the channel stride must be 1 and every row 16-byte
 * aligned (a 16-byte aligned base, the other strides multiples of 8), so the three slices of one packed (B, L, 3, H, D)
 * tensor are read in place.  out: (B, L, H, D) dense in the input dtype, 16-byte aligned; lse: (B, H, L) dense f32.
 * out_lo: NULL (no backward will follow), or a second buffer like out that receives what out's rounding dropped of the f32
 * result, rounded to the same dtype: out + out_lo carries 16 (bf16) or 22 (fp16) bits of it.
 * backward: dout through its four strides under the same rule; out, out_lo and lse as forward wrote them (out_lo NULL: delta
 * from out alone, whose rounding then shows in dq and dk wherever K or Q has a mean); dq, dk, dv written through
 * their strides (the three slices of one packed gradient, say); scratch: gdr_attn_tiled_scratch_bytes(a) bytes, 4-byte
 * aligned (delta_i = sum_d dO_id (O_id + Olo_id)).  Scores, softmax statistics and every accumulation are f32; P and dS are rounded to the
 * 16-bit dtype only as MFMA operands.  Nothing outside [0, B) x [0, L) of any operand is read or written.
 * Envelope: D == 64, GDR_F16 / GDR_BF16, 1 <= L <= GDR_ATTN_TILED_MAX_SEQLEN, B and H >= 1, B * H * L < 2^31, a finite scale;
 * anything else is refused (GDR_ERR_INVALID_ARG, gdr_last_error names the argument) before any launch.  Forward: 1 launch;
 * backward: 3 (delta, the key-stationary dK / dV kernel, the query-stationary dQ kernel).  No atomics and no hand-off between
 * workgroups: two runs are bitwise equal.  No host synchronisation. */
#define GDR_ATTN_TILED_MAX_SEQLEN 16384
typedef struct gdr_attn_tiled_args {
    int32_t B, L, H, D;
    int32_t dtype, reserved;         /* GDR_F16 / GDR_BF16 */
    float scale, reserved2;          /* softmax scale (the caller resolves the default D^-0.5) */
} gdr_attn_tiled_args;
size_t gdr_attn_tiled_scratch_bytes(const gdr_attn_tiled_args* a);   /* 0: the arguments are refused (gdr_last_error) */
int gdr_attn_tiled_forward(const gdr_attn_tiled_args* a, const void* q, const int64_t* q_strides, const void* k,
                           const int64_t* k_strides, const void* v, const int64_t* v_strides, void* out, void* out_lo,
                           float* lse, void* stream);
int gdr_attn_tiled_backward(const gdr_attn_tiled_args* a, const void* dout, const int64_t* dout_strides, const void* q,
                            const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                            const int64_t* v_strides, const void* out, const void* out_lo, const float* lse, void* dq,
                            const int64_t* dq_strides, void* dk, const int64_t* dk_strides, void* dv, const int64_t* dv_strides,
                            void* scratch, void* stream);

/* ---- point serialization for the point decoder (csrc/serialize.hip; added in v17, backward-compatible) ------------------
 * What the reference's Point.serialization and SerializedAttention.get_padding_and_inverse compute with tensor ops: the
 * space-filling-curve code of every point's grid cell under up to GDR_SERIAL_MAX_ORDERS orders, the stable argsort of each
 * code row with its inverse permutation, and the pad / unpad / cu_seqlens tables of the patch attention.  The code
 * semantics are restated in the header of csrc/serialize.hip.  The caller owns every buffer; all of them are device memory
 * except `strides` and `orders`.  Refusals happen before any launch; no entry point synchronises with the host.
 *
 * encode: grid_coord (N, 3) int32 or int64 read through its two element strides; batch: N dense int64 or NULL; code: (k, N)
 *   dense int64, row r under orders[r] (any of the four, repeats allowed).  1 <= depth <= 16; coordinates are taken modulo
 *   2^depth.  One launch.
 * decode: order GDR_SERIAL_Z or GDR_SERIAL_HILBERT; code: N dense int64 -> grid_coord (N, 3) dense int64 and batch
 *   (= code >> 3 * depth), N dense int64.
 * sort: least-significant-digit radix sort of the k rows of `code` on their `bits` low bits (1..63; higher bits must be
 *   equal within a row), 32-bit indices inside.  order, inverse: (k, N) dense int64 with code[r, order[r, j]] non-decreasing
 *   in j, equal codes in ascending point index, and inverse[r, order[r, j]] = j.  workspace: gdr_serial_sort_bytes(k, N)
 *   bytes, 256-byte aligned.  3 * ceil(bits / 8) launches.
 * patch_tables: offset: the B segment ends off_1 <= ... <= off_B (off_0 = 0 is implied), patch size P.  Segment i has n_i
 *   points and the padded length m_i = n_i if n_i <= P, else ceil(n_i / P) * P; poff is the exclusive prefix sum of the m_i.
 *   unpad[j] = j + poff_i - off_i for point j of segment i; pad[t] = off_i + (l if l < n_i else l - P), l = t - poff_i, for
 *   padded slot t of segment i; cu_seqlens = for every i the values poff_i, poff_i + P, ... below poff_(i+1), then the padded
 *   total.  The caller gives the sizes of its buffers — N = off_B entries of unpad, `total` entries of pad, n_seq + 1 entries
 *   of cu_seqlens — and nothing is written beyond them whatever the offsets on the device say.  One launch. */
#define GDR_SERIAL_Z 0
#define GDR_SERIAL_Z_TRANS 1
#define GDR_SERIAL_HILBERT 2
#define GDR_SERIAL_HILBERT_TRANS 3
#define GDR_SERIAL_MAX_ORDERS 8
#define GDR_SERIAL_MAX_DEPTH 16
#define GDR_SERIAL_MAX_POINTS (1 << 30)
#define GDR_SERIAL_SORT_TILE 1024      /* keys per workgroup of the sort */
#define GDR_SERIAL_MAX_SEGMENTS 1024
int gdr_serial_encode(const void* grid_coord, const int64_t* strides, int32_t coord_is_int64, const int64_t* batch, int64_t N,
                      int32_t depth, int32_t k, const int32_t* orders, int64_t* code, void* stream);
int gdr_serial_decode(const int64_t* code, int64_t N, int32_t depth, int32_t order, int64_t* grid_coord, int64_t* batch,
                      void* stream);
size_t gdr_serial_sort_bytes(int32_t k, int64_t N);   /* 0: the arguments are refused (gdr_last_error) */
int gdr_serial_sort(const int64_t* code, int32_t k, int64_t N, int32_t bits, void* workspace, size_t workspace_bytes,
                    int64_t* order, int64_t* inverse, void* stream);
int gdr_serial_patch_tables(const int64_t* offset, int32_t B, int32_t P, int64_t N, int64_t total, int32_t n_seq, int64_t* pad,
                            int64_t* unpad, int32_t* cu_seqlens, void* stream);

/* ---- projected bilinear sampling of point and volume features (csrc/pointfeat.hip; added in v17, backward-compatible) -----
 * What the reference's Network.get_point_feats and Network.build_feat_vol compute with tensor ops (projection, cat, einsum,
 * F.grid_sample with zero padding, |depth sample - z|); the arithmetic is restated in the header of csrc/pointfeat.hip.
 * fp32 only.  The caller owns every buffer; all are device memory except `a` and the stride arrays (int64 element strides,
 * one per dimension of the tensor they follow).  w2cs (V, 4, 4) and ixts (V, 3, 3) are dense and receive no gradient.
 * Refusals happen before any launch; N = 0 returns GDR_OK without one; no entry point synchronises with the host.
 *
 * point_feats: img_ref (V, 3, H, W), image (V, H, W, 3), acc_map (V, H, W), depth (V, H, W[, 1]: three strides), points
 *   (N, 3); out (N, V, 8) dense, 16-byte aligned: ref rgb, render rgb, acc, |depth sample - z|.  One launch.
 * point_feats backward: grad_out (N, V, 8) dense.  grad_img_ref / grad_image / grad_acc_map / grad_depth: dense tensors of
 *   the sources' shapes that the caller ZERO-FILLED (float atomics add into them); grad_points (N, 3) dense, written with
 *   plain stores (bitwise reproducible).  A NULL gradient pointer means "not wanted": nothing is issued for it, and a source
 *   whose values no wanted gradient needs may be NULL too (img_ref, image and acc_map unless grad_points is given).
 * sample_views: images (V, C, H, W), points (N, 3); out (V, C, N) and z (V, N) dense.  One launch.
 * sample_views backward: grad_out (V, C, N) dense, grad_z (V, N) dense or NULL (= zeros); grad_images (V, C, H, W) dense and
 *   zero-filled by the caller, grad_points (N, 3) dense; NULL = not wanted, as above.  One launch. */
#define GDR_PF_MAX_VIEWS 16
#define GDR_PF_MAX_CHANNELS 4096
#define GDR_PF_MAX_SIDE 16384
#define GDR_PF_MAX_POINTS INT64_C(0x7fffffff)
typedef struct gdr_pointfeat_args {
    int64_t N;               /* points */
    int32_t V, C, H, W;      /* views, channels (sample_views only), image size */
    int32_t reserved;
} gdr_pointfeat_args;
int gdr_point_feats_forward(const gdr_pointfeat_args* a, const float* img_ref, const int64_t* img_ref_strides, const float* image,
                            const int64_t* image_strides, const float* acc_map, const int64_t* acc_map_strides,
                            const float* depth, const int64_t* depth_strides, const float* points, const int64_t* points_strides,
                            const float* w2cs, const float* ixts, float* out, void* stream);
int gdr_point_feats_backward(const gdr_pointfeat_args* a, const float* grad_out, const float* img_ref,
                             const int64_t* img_ref_strides, const float* image, const int64_t* image_strides,
                             const float* acc_map, const int64_t* acc_map_strides, const float* depth,
                             const int64_t* depth_strides, const float* points, const int64_t* points_strides, const float* w2cs,
                             const float* ixts, float* grad_img_ref, float* grad_image, float* grad_acc_map, float* grad_depth,
                             float* grad_points, void* stream);
int gdr_sample_views_forward(const gdr_pointfeat_args* a, const float* images, const int64_t* images_strides, const float* points,
                             const int64_t* points_strides, const float* w2cs, const float* ixts, float* out, float* z,
                             void* stream);
int gdr_sample_views_backward(const gdr_pointfeat_args* a, const float* grad_out, const float* grad_z, const float* images,
                              const int64_t* images_strides, const float* points, const int64_t* points_strides,
                              const float* w2cs, const float* ixts, float* grad_images, float* grad_points, void* stream);

/* ---- submanifold sparse 3-D convolution (csrc/subm_conv.hip; added in v17, backward-compatible) ---------------------------
 * The one spconv layer of the reference's point decoder (spconv.SubMConv3d, stride 1): a neighbour table per (coordinates,
 * kernel size), then out[i] = bias + sum_k feat[nbr[k, i]] @ W[k] and its three gradients.  The semantics are restated in the
 * header of csrc/subm_conv.hip.  The caller owns every buffer; all are device memory except `a`, `spatial_shape` and `ksize`.
 * Refusals happen before any launch; N = 0 returns GDR_OK without one; no entry point synchronises with the host.
 *
 * build_table: indices (N, 4) int32 dense, 16-byte aligned: (batch, c0, c1, c2).  spatial_shape[3] >= 1, batch_size >= 1,
 *   ksize[3] each 1, 3 or 5: K = ksize[0] * ksize[1] * ksize[2] <= GDR_SUBM_MAX_TAPS taps, tap k = (t0 * ksize[1] + t1) *
 *   ksize[2] + t2.  nbr (K, N) int32: nbr[k, i] = the site at coord_i + (t0, t1, t2) - ksize / 2 in site i's batch, or -1.
 *   Sites that share a voxel: a lookup answers the LOWEST point index among them; rep (N) int32 is that index for site i's own
 *   voxel.  A site with batch >= batch_size or a coordinate outside spatial_shape is never found, has nbr[., i] = -1 and
 *   rep[i] = i; nothing is read or written out of bounds whatever `indices` holds.  order (N) int32: the sites by ascending
 *   voxel key ((b S0 + c0) S1 + c1) S2 + c2, equal keys by ascending point index (the runs the backward sums over).
 *   workspace: gdr_subm_table_bytes(N), 256-byte aligned.  2 launches + gdr_serial_sort on the key's bits; every device
 *   loop has a trip count the host knows (ceil(log2 N) + 1 search steps).
 * forward: feat (N, Cin) through its row stride (elements; channels unit-stride), weight (Cout, k0, k1, k2, Cin) dense and
 *   16-byte aligned (spconv 2.x's parameter layout), bias (Cout) or NULL, out (N, Cout) dense and 16-byte aligned; all of
 *   a->dtype.  Cross-correlation, f32 accumulation (MFMA), one launch, no atomics: two runs are bitwise equal.
 * backward: grad_out (N, Cout) dense of a->dtype.  grad_feat (N, Cin) dense of a->dtype; grad_weight (Cout, K, Cin) and
 *   grad_bias (Cout) dense f32.  A NULL output pointer means "not wanted": nothing is issued for it.  With G = the sum of
 *   grad_out over each voxel's sites, kept at the representative: grad_feat[j] = sum_k G[nbr[K-1-k, j]] @ W[k]^T for
 *   representatives and zero rows for the rest, grad_weight[k] = sum_r feat[nbr[k, r]]^T @ G[r], grad_bias = column sums of
 *   grad_out.  workspace: gdr_subm_backward_bytes(a), 256-byte aligned.  No atomics: two runs are bitwise equal.
 * Envelope: Cin, Cout multiples of 8 in 8..GDR_SUBM_MAX_CHANNELS, 0 <= N <= GDR_SUBM_MAX_POINTS (the sort's limit). */
#define GDR_SUBM_F16 GDR_F16
#define GDR_SUBM_BF16 GDR_BF16
#define GDR_SUBM_F32 GDR_F32
#define GDR_SUBM_MAX_TAPS 125
#define GDR_SUBM_MAX_CHANNELS 512
#define GDR_SUBM_MAX_POINTS (1 << 30)
typedef struct gdr_subm_args {
    int32_t N, Cin, Cout, K;     /* sites, channels, taps */
    int32_t dtype, reserved;     /* GDR_SUBM_F16 / GDR_SUBM_BF16 / GDR_SUBM_F32 */
} gdr_subm_args;
size_t gdr_subm_table_bytes(int64_t N);   /* 0: the arguments are refused (gdr_last_error) */
int gdr_subm_build_table(const int32_t* indices, int64_t N, const int32_t* spatial_shape, int32_t batch_size, const int32_t* ksize,
                         void* workspace, size_t workspace_bytes, int32_t* nbr, int32_t* rep, int32_t* order, void* stream);
int gdr_subm_conv_forward(const gdr_subm_args* a, const void* feat, int64_t feat_stride, const int32_t* nbr, const void* weight,
                          const void* bias, void* out, void* stream);
size_t gdr_subm_backward_bytes(const gdr_subm_args* a);   /* 0: the arguments are refused (gdr_last_error) */
int gdr_subm_conv_backward(const gdr_subm_args* a, const void* grad_out, const void* feat, int64_t feat_stride, const int32_t* nbr,
                           const int32_t* rep, const int32_t* order, const void* weight, void* workspace, size_t workspace_bytes,
                           void* grad_feat, float* grad_weight, float* grad_bias, void* stream);

/* ---- CSR segment reductions for the point decoder (csrc/segment.hip; added in v17, backward-compatible) ------------------
 * What the reference takes from torch_scatter and torch_geometric.utils: segment_csr, gather_csr, the scatter_* family (by a
 * stable sort of the index, gdr_serial_sort, and the same kernels) and the pieces of a segment softmax.  The semantics are
 * restated in the header of csrc/segment.hip.  The caller owns every buffer; all are device memory.  Refusals happen before
 * any launch; no entry point synchronises with the host.  No atomics: two runs are bitwise equal.  Every indptr value is
 * clamped to [0, N] where it is read and a segment with end < start is empty, so a malformed indptr gives unspecified values
 * and never an access outside the buffers.  0 <= N, S <= 2^31 - 2, 1 <= C <= GDR_SEG_MAX_CHANNELS.
 *
 * reduce: src (N, C) of `dtype` through its row stride (elements; channels unit-stride); perm: NULL or N int64 (logical row r
 *   reads src[perm[r]]); indptr: S + 1 int64; out (S, C) dense, 16-byte aligned, of `dtype`: out[s] = op over the logical rows
 *   indptr[s] .. indptr[s + 1] - 1.  f16 / bf16 / f32 accumulate in f32; GDR_SEG_I64 takes GDR_SEG_SUM only.  min / max also
 *   write arg (S, C) int64: the src row that won, the lowest logical row on ties.  An empty segment gives 0 and arg = N; mean
 *   divides by max(count, 1).  workspace: gdr_seg_reduce_bytes(N, S, C) bytes, 256-byte aligned.  2 launches.
 * gather: src (S, C) through its row stride, out (N, C) dense: out[perm ? perm[r] : r] = src[s] for every logical row r of
 *   segment s, divided by max(count, 1) if inv_count.  Rows in no segment are zero-filled if fill_outside, else untouched.
 *   The forward of gather_csr and the backward of sum / mean.  1 launch.
 * route: grad_src (N, C) dense = 0, then grad_src[arg[s, c], c] = grad_out[s, c] where 0 <= arg < N; grad_out, arg (S, C)
 *   dense.  The backward of min / max (floating dtypes).  A memset and 1 launch.
 * ptr_from_sorted: indptr[s] = the first position i in [0, N] with index[perm ? perm[i] : i] >= s, for s = 0 .. S (S + 1 int64
 *   written); the index must be non-decreasing in that order.  1 launch. */
#define GDR_SEG_ROWS 32                /* rows per run of the reduce and the gather */
#define GDR_SEG_MAX_CHANNELS 65536
#define GDR_SEG_F16 GDR_F16
#define GDR_SEG_BF16 GDR_BF16
#define GDR_SEG_F32 GDR_F32
#define GDR_SEG_I64 3
#define GDR_SEG_SUM 0
#define GDR_SEG_MEAN 1
#define GDR_SEG_MIN 2
#define GDR_SEG_MAX 3
size_t gdr_seg_reduce_bytes(int64_t N, int64_t S, int32_t C);   /* 0: the arguments are refused (gdr_last_error) */
int gdr_seg_reduce(const void* src, int64_t src_stride, const int64_t* perm, const int64_t* indptr, int64_t N, int64_t S,
                   int32_t C, int32_t dtype, int32_t op, void* workspace, size_t workspace_bytes, void* out, int64_t* arg,
                   void* stream);
int gdr_seg_gather(const void* src, int64_t src_stride, const int64_t* indptr, const int64_t* perm, int64_t N, int64_t S,
                   int32_t C, int32_t dtype, int32_t inv_count, int32_t fill_outside, void* out, void* stream);
int gdr_seg_route(const void* grad_out, const int64_t* arg, int64_t N, int64_t S, int32_t C, int32_t dtype, void* grad_src,
                  void* stream);
int gdr_seg_ptr_from_sorted(const int64_t* index, const int64_t* perm, int64_t N, int64_t S, int64_t* indptr, void* stream);

/* ---- fused row normalisations of the point decoder (csrc/norm.hip; added in v17, backward-compatible) ----------------------
 * ada: the reference's AdaLayerNorm, out[i] = scale[b] * layer_norm(feat[i]) for row i of segment b; pe: the input of
 * UpscaleModule.delta_f, layer_norm([sin(f x), cos(f x), feat of the parent]).  The arithmetic is restated in the header of
 * csrc/norm.hip.  The caller owns every buffer; all are device memory.  Every `*_dtype` is one of GDR_NORM_F16 / BF16 / F32
 * and the types of one call are independent; the arithmetic is f32.  Refusals happen before any launch; N = 0 / P = 0 return
 * GDR_OK without one; no entry point allocates or synchronises with the host.  No atomics: two runs are bitwise equal.
 * Envelope (GDR_ERR_UNSUPPORTED beyond it): C a multiple of 8 in 8..GDR_NORM_MAX_CHANNELS, 1 <= B <= GDR_NORM_MAX_SEGMENTS,
 * 1 <= F <= GDR_NORM_MAX_FREQS, 1 <= S <= GDR_NORM_MAX_UPSCALE, N and P * S below 2^31.
 * Rows: "rows of X" below means a 16-byte aligned base and a row stride (in elements) that is a multiple of 8 and >= the row.
 *
 * ada_forward: rows of feat (N, C) and scale (B, C); offset: B int64, the inclusive segment ends (non-decreasing; values are
 *   clamped to [0, N] where they are read); out (N, C) dense, 16-byte aligned, of out_dtype.  Rows at or behind offset[B - 1]
 *   are written as zeros.  1 launch.
 * ada_backward: grad_out: rows of (N, C) of grad_dtype.  grad_feat (N, C) dense of feat_dtype, grad_scale (B, C) dense of
 *   scale_dtype, both 16-byte aligned and written whole (rows behind the last end and empty segments get zeros).  mean and rstd
 *   are recomputed.  workspace: gdr_norm_ada_backward_bytes(N, B, C) bytes, 256-byte aligned.  2 launches.
 * pe_forward: x (P * S, 3) dense; rows of feat (P, C); freq: F values; out: rows of (P * S, 6 F + C) through out_stride; the
 *   elements of a row behind 6 F + C up to the next multiple of 8 are written as zeros.  1 launch.
 * pe_backward: grad_out (P * S, 6 F + C) through grad_stride, which must be even, from a base aligned to two elements (a
 *   16-byte base and a stride that is a multiple of 8 take the wide path).  grad_x (P * S, 3) dense of x_dtype, grad_feat
 *   (P, C) dense of feat_dtype, 16-byte aligned; a NULL output is not wanted.  1 launch. */
#define GDR_NORM_F16 GDR_F16
#define GDR_NORM_BF16 GDR_BF16
#define GDR_NORM_F32 GDR_F32
#define GDR_NORM_ROWS 32               /* rows per workgroup of the ada backward: one dscale partial pair per that many rows */
#define GDR_NORM_MAX_CHANNELS 1024
#define GDR_NORM_MAX_SEGMENTS 1024
#define GDR_NORM_MAX_FREQS 16
#define GDR_NORM_MAX_UPSCALE 16
int gdr_norm_ada_forward(const void* feat, int64_t feat_stride, int32_t feat_dtype, const void* scale, int64_t scale_stride,
                         int32_t scale_dtype, const int64_t* offset, int64_t N, int32_t B, int32_t C, float eps, void* out,
                         int32_t out_dtype, void* stream);
size_t gdr_norm_ada_backward_bytes(int64_t N, int32_t B, int32_t C);   /* 0: the arguments are refused (gdr_last_error) */
int gdr_norm_ada_backward(const void* grad_out, int64_t grad_stride, int32_t grad_dtype, const void* feat, int64_t feat_stride,
                          int32_t feat_dtype, const void* scale, int64_t scale_stride, int32_t scale_dtype, const int64_t* offset,
                          int64_t N, int32_t B, int32_t C, float eps, void* workspace, size_t workspace_bytes, void* grad_feat,
                          void* grad_scale, void* stream);
int gdr_norm_pe_forward(const void* x, int32_t x_dtype, const void* feat, int64_t feat_stride, int32_t feat_dtype, const void* freq,
                        int32_t freq_dtype, int64_t P, int32_t S, int32_t C, int32_t F, float eps, void* out, int64_t out_stride,
                        int32_t out_dtype, void* stream);
int gdr_norm_pe_backward(const void* grad_out, int64_t grad_stride, int32_t grad_dtype, const void* x, int32_t x_dtype,
                         const void* feat, int64_t feat_stride, int32_t feat_dtype, const void* freq, int32_t freq_dtype, int64_t P,
                         int32_t S, int32_t C, int32_t F, float eps, void* grad_x, void* grad_feat, void* stream);

/* ---- UpscaleModule's glue round its Linears (csrc/upscale.hip; backward-compatible additions to v17) -------------------------
 * expand: from t = delta_x(in_f) to the child coordinates and the input of delta_f; merge: skip row + drop-path branch +
 * AdaLayerNorm.  The arithmetic is restated in the header of csrc/upscale.hip; the row passes are norm.hip's (one source).
 * The caller owns every buffer; all are device memory.  Every `*_dtype` is one of GDR_NORM_F16 / BF16 / F32 and the types of
 * one call are independent; the arithmetic is f32.  Refusals happen before any launch; N = 0 returns GDR_OK without one; no
 * entry point allocates or synchronises with the host.  No atomics: two runs are bitwise equal.  Envelope: norm's, with
 * N (parents) and N * S below 2^31.  "Rows" as above.
 *
 * expand_forward: t (N, 3 S) dense; coord (N, 3) dense; rows of feat (N, C); freq: F values; half_grid = 0.5 * grid_size;
 *   out_x (N S, 3) dense of out_x_dtype; h: rows of (N S, 6 F + C) through h_stride, padded with zeros to a multiple of 8.
 *   1 launch.
 * expand_backward: grad_h as pe_backward's grad_out, or NULL (zeros); grad_out_x (N S, 3) dense of out_x_dtype, or NULL (zeros);
 *   grad_t (N, 3 S) of t_dtype, grad_coord (N, 3) of coord_dtype, grad_feat (N, C) dense of feat_dtype, 16-byte aligned; a NULL
 *   output is not wanted and not stored.  1 launch.
 * merge_forward: rows of skip (N, C), branch (N S, C), scale (B, C); keep: N S values or NULL (ones); offset: B int64, the
 *   PARENTS' inclusive segment ends (clamped to [0, N] where they are read); out (N S, C) dense, 16-byte aligned; the rows of
 *   parents at or behind offset[B - 1] are zeros.  1 launch.
 * merge_backward: grad_out: rows of (N S, C).  grad_skip (N, C) of skip_dtype, grad_branch (N S, C) of branch_dtype, grad_scale
 *   (B, C) of scale_dtype, dense, 16-byte aligned, written whole; a NULL output is not wanted and not stored.  workspace:
 *   gdr_upscale_merge_backward_bytes(N, S, B, C) bytes, 256-byte aligned.  1 launch + the fold when grad_scale is wanted. */
int gdr_upscale_expand_forward(const void* t, int32_t t_dtype, const void* coord, int32_t coord_dtype, const void* feat,
                               int64_t feat_stride, int32_t feat_dtype, const void* freq, int32_t freq_dtype, int64_t N, int32_t S,
                               int32_t C, int32_t F, float half_grid, int32_t absolute_pe, float eps, void* out_x, int32_t out_x_dtype,
                               void* h, int64_t h_stride, int32_t h_dtype, void* stream);
int gdr_upscale_expand_backward(const void* grad_h, int64_t grad_h_stride, int32_t grad_h_dtype, const void* grad_out_x,
                                int32_t out_x_dtype, const void* t, int32_t t_dtype, const void* coord, int32_t coord_dtype,
                                const void* feat, int64_t feat_stride, int32_t feat_dtype, const void* freq, int32_t freq_dtype,
                                int64_t N, int32_t S, int32_t C, int32_t F, float half_grid, int32_t absolute_pe, float eps,
                                void* grad_t, void* grad_coord, void* grad_feat, void* stream);
int gdr_upscale_merge_forward(const void* skip, int64_t skip_stride, int32_t skip_dtype, const void* branch, int64_t branch_stride,
                              int32_t branch_dtype, const void* keep, int32_t keep_dtype, const void* scale, int64_t scale_stride,
                              int32_t scale_dtype, const int64_t* offset, int64_t N, int32_t S, int32_t B, int32_t C, float eps,
                              void* out, int32_t out_dtype, void* stream);
size_t gdr_upscale_merge_backward_bytes(int64_t N, int32_t S, int32_t B, int32_t C);   /* 0: the arguments are refused */
int gdr_upscale_merge_backward(const void* grad_out, int64_t grad_stride, int32_t grad_dtype, const void* skip, int64_t skip_stride,
                               int32_t skip_dtype, const void* branch, int64_t branch_stride, int32_t branch_dtype, const void* keep,
                               int32_t keep_dtype, const void* scale, int64_t scale_stride, int32_t scale_dtype, const int64_t* offset,
                               int64_t N, int32_t S, int32_t B, int32_t C, float eps, void* workspace, size_t workspace_bytes,
                               void* grad_skip, void* grad_branch, void* grad_scale, void* stream);

/* ---- the residual junctions of the point decoder's Block (csrc/block.hip; backward-compatible additions to v17) ---------------
 * One launch for what lies between a Block's conv / attention / MLP and the next Linear: a norm of the branch, the drop-path
 * product, the residual sum, the next norm.  The arithmetic is restated in the header of csrc/block.hip; statistics, mapping
 * and ada's segment rules and fold are norm.hip's (one source).  The caller owns every buffer; all are device memory.  Every
 * `*_dtype` is one of GDR_NORM_F16 / BF16 / F32 and the types of one call are independent; the arithmetic is f32.  Refusals
 * happen before any launch; N = 0 launches no row kernel; no entry point allocates or synchronises with the host.  No atomics:
 * two runs are bitwise equal.  Envelope: norm's (C, B, N below 2^31).  "Rows" as above.
 *
 * GdrBlockNorm describes one norm (NULL = GDR_BLOCK_NORM_NONE).  LN: no parameters.  LN_AFFINE: w = weight (C) or NULL (ones),
 *   b = bias (C) or NULL (zeros), 16-byte aligned.  ADA: w = rows of scale (B, C) through w_stride, and `offset` (B int64
 *   inclusive segment ends, clamped to [0, N] where read) is required.  grad_w / grad_b are read by the backward only: dense
 *   outputs of w's / b's shape and dtype, written whole; NULL = not wanted and not stored.
 * junction_forward: rows of skip and branch (N, C); keep: N values or NULL (ones); b0 = pre(branch) rounded to pre_out_dtype,
 *   keep * b0 rounded to kept_dtype, y = skip + that rounded to y_dtype; y (N, C) dense, 16-byte aligned, every row written;
 *   n = post(y) (N, C) dense of n_dtype, ignored when post is none.  1 launch.
 * junction_backward: grad_y / grad_n: rows of (N, C), or NULL (zeros); grad_skip (N, C) of skip_dtype, grad_branch (N, C) of
 *   branch_dtype, dense, 16-byte aligned, written whole; NULL = not wanted and not stored.  workspace:
 *   gdr_block_junction_backward_bytes(N, B, C) bytes, 256-byte aligned.  1 launch + one fold per norm whose parameter
 *   gradient is wanted. */
#define GDR_BLOCK_NORM_NONE 0
#define GDR_BLOCK_NORM_LN 1
#define GDR_BLOCK_NORM_LN_AFFINE 2
#define GDR_BLOCK_NORM_ADA 3
typedef struct GdrBlockNorm {
    int32_t kind;          /* GDR_BLOCK_NORM_* */
    int32_t w_dtype, b_dtype;
    float eps;
    const void* w;
    const void* b;
    int64_t w_stride;
    void* grad_w;
    void* grad_b;
} GdrBlockNorm;
int gdr_block_junction_forward(const void* skip, int64_t skip_stride, int32_t skip_dtype, const void* branch, int64_t branch_stride,
                               int32_t branch_dtype, const void* keep, int32_t keep_dtype, const GdrBlockNorm* pre,
                               const GdrBlockNorm* post, const int64_t* offset, int64_t N, int32_t B, int32_t C, int32_t pre_out_dtype,
                               int32_t kept_dtype, void* y, int32_t y_dtype, void* n, int32_t n_dtype, void* stream);
size_t gdr_block_junction_backward_bytes(int64_t N, int32_t B, int32_t C);   /* 0: the arguments are refused */
int gdr_block_junction_backward(const void* grad_y, int64_t grad_y_stride, int32_t grad_y_dtype, const void* grad_n,
                                int64_t grad_n_stride, int32_t grad_n_dtype, const void* skip, int64_t skip_stride, int32_t skip_dtype,
                                const void* branch, int64_t branch_stride, int32_t branch_dtype, const void* keep, int32_t keep_dtype,
                                const GdrBlockNorm* pre, const GdrBlockNorm* post, const int64_t* offset, int64_t N, int32_t B, int32_t C,
                                int32_t pre_out_dtype, int32_t kept_dtype, int32_t y_dtype, void* workspace, size_t workspace_bytes,
                                void* grad_skip, void* grad_branch, void* stream);

/* ---- densification masks of the point decoder (csrc/densify.hip; added in v17, backward-compatible) ------------------------
 * What the reference's MaskModule / MaskResModule do around their scores: per-segment top-k / top-p selection, the
 * straight-through gate and the split into selected and remaining rows.  The rules are restated in the header of
 * csrc/densify.hip.  The caller owns every buffer; all are device memory.  Every `*_dtype` is one of GDR_NORM_F16 / BF16 / F32.
 * Refusals happen before any launch; no entry point allocates or synchronises with the host.  No atomics: two runs are
 * bitwise equal.  Envelope (GDR_ERR_UNSUPPORTED beyond it): N <= 2^30, 1 <= B <= GDR_DENSIFY_MAX_SEGMENTS, C a multiple of 8
 * in 8..GDR_DENSIFY_MAX_CHANNELS.  "rows of X" means a 16-byte aligned base and a row stride (elements) that is a multiple of
 * 8 and >= C.
 *
 * select: x: N dense values of x_dtype; offset: B int64 segment ends, clamped on the device to [previous end, N]; mask: N
 *   bytes (0 / 1), written whole; new_offset: B int64.  Rows of a segment are ranked by descending value (NaN first, -0 = +0,
 *   ties by ascending row).  GDR_DENSIFY_TOP_K selects the first min(k_b, n_b) ranks, k_b = ceil(ratio * n_b) with both the
 *   count and the product rounded to x_dtype; GDR_DENSIFY_TOP_P selects rank j iff the inclusive f32 prefix sum of the ranked
 *   values, rounded to x_dtype, is <= threshold (the caller's ratio rounded to x_dtype).  Rows at or behind the last end are
 *   never selected.  workspace: gdr_densify_select_bytes(N, B) bytes, 256-byte aligned.  3 (top-k) or 8 (top-p) launches +
 *   gdr_serial_sort on 32 / 19 / 16 (f32 / f16 / bf16) + bits(B) key bits.
 * gate_forward: rows of feat (N, C); mask NULL or N bytes; out (N, C) dense of out_dtype = feat, or zero where mask is 0.
 * split_scan: dest[i] = the number of rows before i with the same mask value, *count = the number of selected rows.
 *   workspace: gdr_densify_split_bytes(N) bytes, 256-byte aligned.  3 launches.
 * split_forward: row i of feat (converted to out_dtype) and of coord (N, coord_elems) dense elements of coord_elem_bytes (1,
 *   2, 4 or 8) goes to row dest[i] of feat_sel / coord_sel (mask 1) or feat_rest / coord_rest (mask 0), all dense.  A row
 *   whose destination is not below n_sel / n_rest, the capacities of the outputs in rows, is dropped.  1 launch.
 * rows_backward: the backward of the gate (dest NULL: the gradient row of row i is row i of grad_sel through grad_stride) and
 *   of the split (row dest[i] of grad_sel / grad_rest, rows of (n, C) of grad_dtype; zero for a dropped row).  grad_feat (N, C)
 *   dense of feat_dtype = prob[i] * g (g if prob is NULL); grad_prob: N of prob_dtype = sum_c feat[i, c] * g[c] in f32;
 *   grad_coord (N, coord_elems) = the coord gradient row.  A NULL output is not wanted.  1 launch. */
#define GDR_DENSIFY_TOP_K 0
#define GDR_DENSIFY_TOP_P 1
#define GDR_DENSIFY_MAX_SEGMENTS 1024
#define GDR_DENSIFY_MAX_CHANNELS 1024
#define GDR_DENSIFY_CHUNK 1024         /* rows per workgroup of the scans */
size_t gdr_densify_select_bytes(int64_t N, int32_t B);   /* 0: the arguments are refused (gdr_last_error) */
int gdr_densify_select(const void* x, int32_t x_dtype, const int64_t* offset, int64_t N, int32_t B, int32_t mode, float ratio,
                       float threshold, void* workspace, size_t workspace_bytes, uint8_t* mask, int64_t* new_offset, void* stream);
int gdr_densify_gate_forward(const void* feat, int64_t feat_stride, int32_t feat_dtype, const uint8_t* mask, int64_t N, int32_t C,
                             void* out, int32_t out_dtype, void* stream);
size_t gdr_densify_split_bytes(int64_t N);               /* 0: the arguments are refused (gdr_last_error) */
int gdr_densify_split_scan(const uint8_t* mask, int64_t N, void* workspace, size_t workspace_bytes, int64_t* dest, int64_t* count,
                           void* stream);
int gdr_densify_split_forward(const uint8_t* mask, const int64_t* dest, int64_t N, int32_t C, const void* feat, int64_t feat_stride,
                              int32_t feat_dtype, const void* coord, int32_t coord_elems, int32_t coord_elem_bytes, int64_t n_sel,
                              int64_t n_rest, void* feat_sel, void* feat_rest, int32_t out_dtype, void* coord_sel, void* coord_rest,
                              void* stream);
int gdr_densify_rows_backward(const uint8_t* mask, const int64_t* dest, int64_t N, int32_t C, const void* grad_sel, const void* grad_rest,
                              int64_t grad_stride, int32_t grad_dtype, int64_t n_sel, int64_t n_rest, const void* feat,
                              int64_t feat_stride, int32_t feat_dtype, const void* prob, int32_t prob_dtype, const void* gcoord_sel,
                              const void* gcoord_rest, int32_t coord_elems, int32_t coord_elem_bytes, void* grad_feat, void* grad_prob,
                              void* grad_coord, void* stream);

/* ---- per-point view cross attention, folded form (csrc/viewattn.hip; added in v17, backward-compatible) ---------------------
 * The core of a single-query multi-head cross attention over the V views of a point, with the key / value projections folded
 * into the query and the output (generativedensification_amd/viewattn.py): s[n, h, v] = scale * <t[n, h], cond[n, v]>,
 * p = softmax_v(s), u[n, h] = sum_v p[n, h, v] * cond[n, v].  The arithmetic and its backward are restated in the header of
 * csrc/viewattn.hip.  The caller owns every buffer; all are device memory.  Every `*_dtype` is one of GDR_NORM_F16 / BF16 / F32
 * and the types of one call are independent; the arithmetic is f32.  Refusals happen before any launch; N = 0 returns GDR_OK
 * without one; no entry point allocates or synchronises with the host; no workspace.  No atomics: two runs are bitwise equal.
 * Envelope (GDR_ERR_UNSUPPORTED beyond it): Ck 4, 8 or 16, 1 <= H <= GDR_VIEWATTN_MAX_HEADS, 1 <= V <= GDR_VIEWATTN_MAX_VIEWS,
 * N <= 2^27, and "rows of X": a 16-byte aligned base and a row stride (in elements) that is a multiple of 8 and >= the row.
 *
 * forward: rows of t (N, H * Ck), cond (N, V * Ck) and out (N, H * Ck, written through out_stride).  1 launch.
 * backward: rows of grad_out (N, H * Ck), t and cond as in the forward; p is recomputed.  grad_t (N, H * Ck) dense of t_dtype and
 *   grad_cond (N, V * Ck) dense of cond_dtype, both 16-byte aligned and written whole.  1 launch. */
#define GDR_VIEWATTN_MAX_HEADS 64
#define GDR_VIEWATTN_MAX_VIEWS 16
int gdr_viewattn_forward(const void* t, int64_t t_stride, int32_t t_dtype, const void* cond, int64_t cond_stride, int32_t cond_dtype,
                         int64_t N, int32_t H, int32_t Ck, int32_t V, float scale, void* out, int64_t out_stride, int32_t out_dtype,
                         void* stream);
int gdr_viewattn_backward(const void* grad_out, int64_t grad_out_stride, int32_t grad_out_dtype, const void* t, int64_t t_stride,
                          int32_t t_dtype, const void* cond, int64_t cond_stride, int32_t cond_dtype, int64_t N, int32_t H, int32_t Ck,
                          int32_t V, float scale, void* grad_t, void* grad_cond, void* stream);

/* ---- group cross attention of the volume transformer (csrc/groupattn.hip; added in v17, backward-compatible) ----------------
 * The core of a multi-head cross attention in which the Lq queries of a group share its Lk keys, and the two LayerNorms that
 * carry a (B, D, H, W, C) volume into patch order and back (generativedensification_amd/groupattn.py):
 * s[m, h, i, j] = scale * <q[m, i, h], k[m, j, h]>, p = softmax_j(s), out[m, i, h] = sum_j p[m, h, i, j] * v[m, j, h].  The
 * arithmetic, its backward and the row map are restated in the header of csrc/groupattn.hip.  The caller owns every buffer;
 * all are device memory.  Every `*_dtype` is one of GDR_NORM_F16 / BF16 / F32 and the types of one call are independent; the
 * arithmetic is f32.  Refusals happen before any launch; M = 0 / B = 0 return GDR_OK without a row launch; no entry point
 * allocates or synchronises with the host.  No atomics: two runs are bitwise equal.
 * Envelope (GDR_ERR_UNSUPPORTED beyond it): Dh 8, 16 or 32, 1 <= H <= GDR_GROUPATTN_MAX_HEADS, 1 <= Lq <=
 * GDR_GROUPATTN_MAX_QUERIES, 1 <= Lk <= GDR_GROUPATTN_MAX_KEYS, M <= 2^24; C a multiple of 8 in 8..GDR_NORM_MAX_CHANNELS,
 * 1 <= bs <= GDR_GROUPATTN_MAX_BLOCK, B D H W below 2^31; and "rows of X": a 16-byte aligned base and a row stride (in
 * elements) that is a multiple of 8 and >= the row.
 *
 * forward: rows of q (M * Lq, H * Dh), k and v (M * Lk, H * Dh), each through its own stride (k and v may be the two halves of
 *   one (M * Lk, 2 H Dh) matrix); out (M * Lq, H * Dh) dense, 16-byte aligned.  1 launch.
 * backward: rows of grad_out (M * Lq, H * Dh); q, k, v as in the forward; p is recomputed.  grad_q dense of q_dtype, grad_k /
 *   grad_v (M * Lk, H * Dh) dense of k_dtype / v_dtype, all 16-byte aligned and written whole.  1 launch.
 * patchify_norm_forward: vol (B, D, H, W, C) dense (a channels-last volume), D, H, W multiples of bs; patches (B G bs^3, C)
 *   dense of patches_dtype = the rows of vol in patch order (rounded when patches_dtype is narrower than vol_dtype); normed,
 *   same shape, of normed_dtype = the LayerNorm over C of the patches as stored.  weight / bias: C values or NULL.  1 launch.
 * norm_unpatchify_forward: patches (B G bs^3, C) dense; vol (B, D, H, W, C) dense of vol_dtype = the LayerNorm of the rows,
 *   each at its voxel.  1 launch.
 * *_backward: grad_vol / grad_patches (the gradient of the input) dense of the input's dtype, written whole; a NULL
 *   grad_normed / grad_patches input is a zero gradient; grad_weight / grad_bias: C values of weight_dtype / bias_dtype or
 *   NULL (not wanted).  workspace: gdr_groupattn_norm_backward_bytes(B D H W, C) bytes, 256-byte aligned: one partial pair per
 *   GDR_GROUPATTN_NORM_ROWS rows.  1 launch for the rows + 1 that folds the partials when a parameter gradient is wanted. */
#define GDR_GROUPATTN_MAX_HEADS 64
#define GDR_GROUPATTN_MAX_QUERIES 64
#define GDR_GROUPATTN_MAX_KEYS 64
#define GDR_GROUPATTN_MAX_BLOCK 8
#define GDR_GROUPATTN_NORM_ROWS 64     /* rows per workgroup of the norm backwards */
int gdr_groupattn_forward(const void* q, int64_t q_stride, int32_t q_dtype, const void* k, int64_t k_stride, int32_t k_dtype,
                          const void* v, int64_t v_stride, int32_t v_dtype, int64_t M, int32_t Lq, int32_t Lk, int32_t H, int32_t Dh,
                          float scale, void* out, int32_t out_dtype, void* stream);
int gdr_groupattn_backward(const void* grad_out, int64_t grad_out_stride, int32_t grad_out_dtype, const void* q, int64_t q_stride,
                           int32_t q_dtype, const void* k, int64_t k_stride, int32_t k_dtype, const void* v, int64_t v_stride,
                           int32_t v_dtype, int64_t M, int32_t Lq, int32_t Lk, int32_t H, int32_t Dh, float scale, void* grad_q,
                           void* grad_k, void* grad_v, void* stream);
int gdr_groupattn_patchify_norm_forward(const void* vol, int32_t vol_dtype, const void* weight, int32_t weight_dtype, const void* bias,
                                        int32_t bias_dtype, int64_t B, int32_t D, int32_t H, int32_t W, int32_t C, int32_t bs, float eps,
                                        void* patches, int32_t patches_dtype, void* normed, int32_t normed_dtype, void* stream);
int gdr_groupattn_norm_unpatchify_forward(const void* patches, int32_t patches_dtype, const void* weight, int32_t weight_dtype,
                                          const void* bias, int32_t bias_dtype, int64_t B, int32_t D, int32_t H, int32_t W, int32_t C,
                                          int32_t bs, float eps, void* vol, int32_t vol_dtype, void* stream);
size_t gdr_groupattn_norm_backward_bytes(int64_t rows, int32_t C);   /* 0: the arguments are refused (gdr_last_error) */
int gdr_groupattn_patchify_norm_backward(const void* grad_normed, int32_t grad_normed_dtype, const void* grad_patches,
                                         int32_t grad_patches_dtype, const void* vol, int32_t vol_dtype, int32_t patches_dtype,
                                         const void* weight, int32_t weight_dtype, int32_t bias_dtype, int64_t B, int32_t D, int32_t H, int32_t W, int32_t C,
                                         int32_t bs, float eps, void* workspace, size_t workspace_bytes, void* grad_vol, void* grad_weight,
                                         void* grad_bias, void* stream);
int gdr_groupattn_norm_unpatchify_backward(const void* grad_vol, int32_t grad_vol_dtype, const void* patches, int32_t patches_dtype,
                                           const void* weight, int32_t weight_dtype, int32_t bias_dtype, int64_t B, int32_t D, int32_t H,
                                           int32_t W, int32_t C, int32_t bs, float eps, void* workspace, size_t workspace_bytes,
                                           void* grad_patches, void* grad_weight, void* grad_bias, void* stream);

/* ---- dense 3x3x3 convolution of channels-last volumes (csrc/conv3d.hip; added in v17, backward-compatible) -------------------
 * The nn.Conv3d(C, C, 3, padding=1) of the volume transformer's blocks on (B, D, H, W, C) rows
 * (generativedensification_amd/conv3d.py): stride 1, zero padding 1, dilation 1, groups 1, cross-correlation;
 * out[voxel][co] = bias[co] + addend[voxel][co] + sum over the 27 taps k and ci of x[voxel + offset_k][ci] * weight[co][ci][k],
 * tap k = (kd * 3 + kh) * 3 + kw, offset_k = (kd, kh, kw) - 1, a voxel outside the volume contributing zero.  The arithmetic
 * and its gradients are restated in the header of csrc/conv3d.hip.  The caller owns every buffer; all are device memory.
 * `dtype` (GDR_NORM_F16 / BF16 / F32) is the compute dtype: the type of x, of the packed weight, of the addend and of the
 * result; sums are f32.  The parameters and their gradients carry dtypes of their own.  Refusals happen before any launch;
 * B = 0 returns GDR_OK without a product launch; no entry point allocates or synchronises with the host.  No atomics: two
 * runs are bitwise equal.
 * Envelope (GDR_ERR_UNSUPPORTED beyond it): Cin and Cout multiples of 8 in 8..GDR_CONV3D_MAX_CHANNELS, B D H W below 2^31, every
 * row buffer dense and 16-byte aligned, a workspace 256-byte aligned.
 *
 * workspace_bytes: the size of one workspace kind for a call of these sizes; no device work; 0: the arguments are refused
 *   (gdr_last_error).  GDR_CONV3D_WS_PACKED: one packed weight (voxels is not read); GDR_CONV3D_WS_GRAD_WEIGHT: the f32 partial
 *   tiles of grad_weight, one (27, Cout, Cin) set per voxel slab; GDR_CONV3D_WS_GRAD_BIAS: the column-sum partials (Cin is not read).
 * pack_weight: weight (Cout, Cin, 3, 3, 3) dense of weight_dtype -> packed, rounded to `dtype`.  mirrored = 0: [k][co][ci], the
 *   forward's operand; mirrored != 0: [26 - k][ci][co], the operand of the input gradient.  1 launch.
 * forward: out (B, D, H, W, Cout) from x (B, D, H, W, Cin) and a packed weight (27, Cout, Cin); bias: Cout values of bias_dtype,
 *   rounded to `dtype`, or NULL; addend: (B, D, H, W, Cout) rows of `dtype` added to the f32 sum before the one rounding, or
 *   NULL.  The input gradient is this call on grad_out with the mirrored weight and Cin / Cout exchanged.  A workgroup owns a
 *   brick of GDR_CONV3D_BRICK_D x _H x _W voxels of one batch item.  1 launch.
 * grad_weight: (Cout, Cin, 3, 3, 3) dense of grad_weight_dtype, written whole, rounded once from the f32 sums.  2 launches.
 * grad_bias: Cout values of grad_bias_dtype = the column sums of grad_out (voxels, Cout).  2 launches. */
#define GDR_CONV3D_MAX_CHANNELS 1024
#define GDR_CONV3D_BRICK_D 4
#define GDR_CONV3D_BRICK_H 4
#define GDR_CONV3D_BRICK_W 8
#define GDR_CONV3D_WS_PACKED 0
#define GDR_CONV3D_WS_GRAD_WEIGHT 1
#define GDR_CONV3D_WS_GRAD_BIAS 2
size_t gdr_conv3d_workspace_bytes(int32_t what, int32_t dtype, int64_t voxels, int32_t Cin, int32_t Cout);
int gdr_conv3d_pack_weight(const void* weight, int32_t weight_dtype, int32_t Cin, int32_t Cout, int32_t mirrored, void* packed,
                           int32_t dtype, void* stream);
int gdr_conv3d_forward(const void* x, int32_t dtype, const void* packed, const void* bias, int32_t bias_dtype, const void* addend,
                       int64_t B, int32_t D, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* out, void* stream);
int gdr_conv3d_grad_weight(const void* x, const void* grad_out, int32_t dtype, int64_t B, int32_t D, int32_t H, int32_t W, int32_t Cin,
                           int32_t Cout, void* workspace, size_t workspace_bytes, void* grad_weight, int32_t grad_weight_dtype,
                           void* stream);
int gdr_conv3d_grad_bias(const void* grad_out, int32_t dtype, int64_t voxels, int32_t Cout, void* workspace, size_t workspace_bytes,
                         void* grad_bias, int32_t grad_bias_dtype, void* stream);

/* ---- [LayerNorm +] 2x transposed convolution of channels-last volumes (csrc/deconv3d.hip; entry points added within v17) -----
 * The nn.LayerNorm(Cin) and nn.ConvTranspose3d(Cin, Cout, kernel_size=2, stride=2) at the tail of the volume transformer
 * (generativedensification_amd/deconv3d.py) on (B, D, H, W, Cin) rows:
 * out[(b, 2d + i, 2h + j, 2w + k)][co] = bias[co] + sum over ci of n[(b, d, h, w)][ci] * weight[ci][co][t], tap t = (i * 2 + j) * 2 + k,
 * n = x, or with has_norm the row's LayerNorm (biased variance, eps inside the root, optional affine) computed in the same
 * kernel and rounded once to the compute dtype (f32 rows: not rounded at all).  The arithmetic and its gradients are restated
 * in the header of csrc/deconv3d.hip.  The caller owns every buffer; all are device memory.  `dtype` (GDR_NORM_F16 / BF16 /
 * F32) is the compute dtype: the type of x, of the packed weight, of grad_out and of the results; sums are f32 (f64 for f32
 * rows).  The parameters and their gradients carry dtypes of their own; the LayerNorm's affine parameters are read as they
 * are, weight and bias rounded to `dtype`.  Refusals happen before any launch; B = 0 returns GDR_OK; no entry point allocates
 * or synchronises with the host.  No atomics: two runs are bitwise equal.
 * Envelope (GDR_ERR_UNSUPPORTED beyond it): Cin a multiple of 8 in 8..GDR_DECONV3D_MAX_CIN, Cout one in
 * 8..GDR_DECONV3D_MAX_COUT, 8 B D H W (the child rows) below 2^31, every row buffer dense and 16-byte aligned, a workspace
 * 256-byte aligned.
 *
 * workspace_bytes: the size of one workspace kind for `rows` = B D H W parent rows; no device work; 0: the arguments are
 *   refused (gdr_last_error).  _WS_PACKED: one packed weight (rows is not read); _WS_GRAD_WEIGHT: the partial tiles of
 *   grad_weight, one (8, Cin, Cout) set per slab of parent rows (a slab is cut per GDR_DECONV3D_SLAB_MIN rows, 8 at most);
 *   _WS_GRAD_BIAS: the column-sum partials of grad_out; _WS_GRAD_INPUT: the per-workgroup column sums behind grad_ln_weight /
 *   grad_ln_bias; _WS_STATS: the (rows, 2) f64 mean and rstd the forward leaves for the backward.
 * pack_weight: weight (Cin, Cout, 2, 2, 2) dense of weight_dtype -> packed, rounded to `dtype`.  transposed = 0: [t][co][ci], the
 *   forward's operand; transposed != 0: [t][ci][co], the operand of grad_input.  1 launch.
 * forward: out (B, 2D, 2H, 2W, Cout).  stats: NULL, or with has_norm a _WS_STATS buffer that receives mean and rstd.  A
 *   workgroup owns GDR_DECONV3D_TILE_ROWS consecutive parent rows.  1 launch.
 * grad_input: grad_x (B, D, H, W, Cin) (or NULL) from grad_out and the transposed packed weight, with has_norm through the
 *   LayerNorm's backward (x and the forward's stats are read); grad_ln_weight / grad_ln_bias: Cin values each, or NULL; the
 *   workspace is read only for them.  1 launch, + 1 for the two sums.
 * grad_weight: (Cin, Cout, 2, 2, 2) dense of grad_weight_dtype, written whole, rounded once.  2 launches.
 * grad_bias: Cout values of grad_bias_dtype = the column sums of grad_out (child_rows = 8 B D H W, Cout).  2 launches. */
#define GDR_DECONV3D_MAX_CIN 1024
#define GDR_DECONV3D_MAX_COUT 256
#define GDR_DECONV3D_TILE_ROWS 64
#define GDR_DECONV3D_SLAB_MIN 4096
#define GDR_DECONV3D_WS_PACKED 0
#define GDR_DECONV3D_WS_GRAD_WEIGHT 1
#define GDR_DECONV3D_WS_GRAD_BIAS 2
#define GDR_DECONV3D_WS_GRAD_INPUT 3
#define GDR_DECONV3D_WS_STATS 4
size_t gdr_deconv3d_workspace_bytes(int32_t what, int32_t dtype, int64_t rows, int32_t Cin, int32_t Cout);
int gdr_deconv3d_pack_weight(const void* weight, int32_t weight_dtype, int32_t Cin, int32_t Cout, int32_t transposed, void* packed,
                             int32_t dtype, void* stream);
int gdr_deconv3d_forward(const void* x, int32_t dtype, const void* packed, const void* bias, int32_t bias_dtype, int32_t has_norm,
                         const void* ln_weight, int32_t ln_weight_dtype, const void* ln_bias, int32_t ln_bias_dtype, double eps, int64_t B,
                         int32_t D, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* stats, void* out, void* stream);
int gdr_deconv3d_grad_input(const void* grad_out, int32_t dtype, const void* packed_t, const void* x, const void* stats, int32_t has_norm,
                            const void* ln_weight, int32_t ln_weight_dtype, int64_t B, int32_t D, int32_t H, int32_t W, int32_t Cin,
                            int32_t Cout, void* workspace, size_t workspace_bytes, void* grad_x, void* grad_ln_weight,
                            int32_t grad_ln_weight_dtype, void* grad_ln_bias, int32_t grad_ln_bias_dtype, void* stream);
int gdr_deconv3d_grad_weight(const void* x, const void* stats, int32_t has_norm, const void* ln_weight, int32_t ln_weight_dtype,
                             const void* ln_bias, int32_t ln_bias_dtype, const void* grad_out, int32_t dtype, int64_t B, int32_t D, int32_t H,
                             int32_t W, int32_t Cin, int32_t Cout, void* workspace, size_t workspace_bytes, void* grad_weight,
                             int32_t grad_weight_dtype, void* stream);
int gdr_deconv3d_grad_bias(const void* grad_out, int32_t dtype, int64_t child_rows, int32_t Cout, void* workspace, size_t workspace_bytes,
                           void* grad_bias, int32_t grad_bias_dtype, void* stream);

/* ---- coarse Gaussian head (csrc/coarsehead.hip; entry points added within v17) ------------------------------------------------
 * Decoder.forward_coarse of the reference and the centres / mask lines behind it (generativedensification_amd/coarsehead.py) on
 * dense (rows, C) rows: Linear(C, C), ReLU, Linear(C, C), ReLU, Linear(C, K P) with P = 3 + sh_dim + 1 + 3 + 4, the split into
 * offset = 2 sigmoid - 1 (3), sh (sh_dim), opacity + opacity_shift (1), scaling + scaling_shift (3), rotation (4) per k, and
 * optionally centers = group_centers[row % N] + offset half_cell and mask = sigmoid(opacity) > threshold, in one launch.  The
 * arithmetic and its gradients are restated in the header of csrc/coarsehead.hip.  `dtype` (GDR_NORM_F16 / BF16 / F32) is the
 * compute dtype: the type of x, of the packed weights and of grad_x; the hidden rows are rounded to it, sums are f32 (f64 for
 * f32 rows); the five outputs, centers and every upstream gradient are dense f32 with E = rows K elements: offset (E, 3),
 * sh (E, sh_dim), scaling (E, 3), rotation (E, 4), opacity (E), centers (E, 3); mask is E bytes of 0 / 1.  Weights are
 * nn.Linear's (out, in), biases and parameter gradients carry dtypes of their own.  The caller owns every buffer; all are
 * device memory.  Refusals happen before any launch; rows = 0 returns GDR_OK; no entry point allocates or synchronises with the
 * host.  No atomics: two runs are bitwise equal.
 * Envelope (GDR_ERR_UNSUPPORTED beyond it): C a multiple of 8 in 8..GDR_COARSEHEAD_MAX_C (both hidden widths are C), K in 1..4,
 * sh_dim one of 3, 12, 27, 48, K P <= GDR_COARSEHEAD_MAX_OUT, rows K below 2^31, x / grad_x / packed 16-byte aligned, a
 * workspace 256-byte aligned.
 *
 * workspace_bytes: the size of one workspace kind; no device work; 0: the arguments are refused (gdr_last_error).
 *   _WS_PACKED_FORWARD / _WS_PACKED_BACKWARD: the packed weights of the forward / the backward (rows is not read);
 *   _WS_PARTIALS: the partial parameter gradients, one set per slab of rows (a slab is cut per GDR_COARSEHEAD_SLAB_MIN rows,
 *   1024 at most).
 * pack: the three weights rounded to `dtype`, zero-padded; backward = 0: the forward's operands, != 0: the backward's.  1 launch.
 * forward: a workgroup owns GDR_COARSEHEAD_TILE_ROWS consecutive rows.  centers (with group_centers (N, 3) f32, N dividing
 *   rows) and mask may each be NULL.  1 launch.
 * backward: recomputes the hidden rows from x; `offset` is the forward's output; any upstream gradient may be NULL (zeros).
 *   grad_x: (rows, C) of `dtype`, or NULL.  workspace: a _WS_PARTIALS buffer that receives the partial parameter gradients,
 *   or NULL when no parameter gradient is needed.  1 launch.
 * fold: the six parameter gradients (any may be NULL) from the partials, added in a fixed order (16 segments of the slabs, each in slab
 *   order, then the segment sums), each rounded once.  1 launch. */
#define GDR_COARSEHEAD_MAX_C 256
#define GDR_COARSEHEAD_MAX_OUT 128
#define GDR_COARSEHEAD_TILE_ROWS 64
#define GDR_COARSEHEAD_SLAB_MIN 1024
#define GDR_COARSEHEAD_WS_PACKED_FORWARD 0
#define GDR_COARSEHEAD_WS_PACKED_BACKWARD 1
#define GDR_COARSEHEAD_WS_PARTIALS 2
size_t gdr_coarsehead_workspace_bytes(int32_t what, int32_t dtype, int64_t rows, int32_t C, int32_t K, int32_t sh_dim);
int gdr_coarsehead_pack(const void* w1, int32_t w1_dtype, const void* w2, int32_t w2_dtype, const void* w3, int32_t w3_dtype, int32_t C,
                        int32_t K, int32_t sh_dim, int32_t backward, void* packed, int32_t dtype, void* stream);
int gdr_coarsehead_forward(const void* x, int32_t dtype, const void* packed, const void* b1, int32_t b1_dtype, const void* b2, int32_t b2_dtype,
                           const void* b3, int32_t b3_dtype, int64_t rows, int64_t N, int32_t C, int32_t K, int32_t sh_dim,
                           double opacity_shift, double scaling_shift, const void* group_centers, double half_cell, double threshold,
                           void* offset, void* sh, void* scaling, void* rotation, void* opacity, void* centers, void* mask, void* stream);
int gdr_coarsehead_backward(const void* x, int32_t dtype, const void* packed, const void* b1, int32_t b1_dtype, const void* b2, int32_t b2_dtype,
                            int64_t rows, int32_t C, int32_t K, int32_t sh_dim, const void* offset, const void* grad_offset, const void* grad_sh,
                            const void* grad_scaling, const void* grad_rotation, const void* grad_opacity, const void* grad_centers,
                            double half_cell, void* grad_x, void* workspace, size_t workspace_bytes, void* stream);
int gdr_coarsehead_fold(const void* workspace, size_t workspace_bytes, int32_t dtype, int64_t rows, int32_t C, int32_t K, int32_t sh_dim,
                        void* grad_w1, int32_t grad_w1_dtype, void* grad_b1, int32_t grad_b1_dtype, void* grad_w2, int32_t grad_w2_dtype,
                        void* grad_b2, int32_t grad_b2_dtype, void* grad_w3, int32_t grad_w3_dtype, void* grad_b3, int32_t grad_b3_dtype,
                        void* stream);

/* ---- fine Gaussian head and fine-set assembly (csrc/finehead.hip; entry points added within v17) -------------------------------
 * The head: `feat2attr` of the reference's GaussianModule / GaussianResModule (generativedensification_amd/finehead.py) on dense
 * (rows, C) rows: Linear(C, C), GELU (exact, erf), Linear(C, P) with P = sh_dim + 1 + 3 + 4.  `dtype` (GDR_NORM_F16 / BF16 / F32)
 * is the compute dtype: the type of x, of the packed weights and of grad_x; z1 and the hidden row are rounded to it, GELU and its
 * derivative are evaluated in f32 (f64 for f32 rows) from the rounded z1, sums are f32 (f64 for f32 rows).  out is (rows, P) dense
 * of out_dtype, the compute dtype or GDR_NORM_F32 (the last layer's sum without a 16-bit rounding); grad_out is (rows, P) dense of
 * grad_out_dtype or NULL (zeros).  Weights are nn.Linear's (out, in); biases and parameter gradients carry dtypes of their own.
 * The caller owns every buffer; all are device memory.  Refusals happen before any launch; rows = 0 returns GDR_OK; no entry
 * point allocates or synchronises with the host.  No atomics: two runs are bitwise equal.  The arithmetic is restated in the
 * header of csrc/finehead.hip.
 * Envelope (GDR_ERR_UNSUPPORTED beyond it): C a multiple of 8 in 8..GDR_FINEHEAD_MAX_C (the hidden width is C), sh_dim one of 3,
 * 12, 27, 48, rows below 2^31, x / grad_x / packed 16-byte aligned, a workspace 256-byte aligned.
 *
 * workspace_bytes: the size of one workspace kind; no device work; 0: the arguments are refused (gdr_last_error).
 *   _WS_PACKED_FORWARD / _WS_PACKED_BACKWARD: the packed weights of the forward / the backward (rows is not read);
 *   _WS_PARTIALS: the partial parameter gradients, one set per slab of rows (a slab is cut per GDR_FINEHEAD_SLAB_MIN rows, 256 at
 *   most).
 * backward_step: the rows a workgroup of the backward takes per step for this shape (64, 32 or 16; 0: refused).
 * pack: both weights rounded to `dtype`, zero-padded; backward = 0: the forward's operands, != 0: the backward's.  1 launch.
 * forward: a workgroup owns GDR_FINEHEAD_TILE_ROWS consecutive rows; the hidden row stays in LDS.  1 launch.
 * backward: recomputes z1 and the hidden row from x.  grad_x: (rows, C) of `dtype`, or NULL.  workspace: a _WS_PARTIALS buffer
 *   that receives the partial parameter gradients, or NULL when no parameter gradient is needed.  1 launch.
 * fold: the four parameter gradients (any may be NULL) from the partials, added in a fixed order (16 segments of the slabs, each
 *   in slab order, then the segment sums), each rounded once.  1 launch.
 *
 * The assembly: the fine Gaussian set of the reference's Network.forward for one sample: the rows of up to
 * GDR_FINEHEAD_MAX_LEVELS decoder levels, then the coarse Gaussians with mask[i] != 0 whose masked row m has selected[m] == 0 (the
 * survivors), in row order.  Outputs, dense f32: centers (T, 3), shs (T, sh_dim), opacity (T, 1), scaling (T, 3), rotation (T, 4)
 * with T = sum of level_rows + n_rest.  A level row gives centers = coord (f32) and, from its attribute row (attr_dtype, P wide,
 * converted to f32 first), shs = the first sh_dim columns, opacity = the next + opacity_shift, scaling = the next 3 +
 * scaling_shift, rotation = the last 4.  A survivor row copies the coarse tensors ((Nc, 3 | 1 | 3 | 4) f32) and shs_fine
 * ((n_masked, sh_dim) f32).  Row counts are below 2^31.
 * scan: rank_masked (Nc) = the number of masked rows before row i, -1 where mask[i] == 0; row_of_masked (n_masked) its inverse;
 *   rank_rest (n_masked) = the number of unselected rows before masked row m, -1 where selected; masked_of_rest (n_masked) its
 *   inverse; count[0] = the masked rows, count[1] = the unselected rows.  Inverse entries nothing maps to are left as they were.
 *   workspace: gdr_finehead_scan_bytes bytes, 256-byte aligned.  3 launches.
 * assemble: n_rest (<= n_masked) survivor rows are written; a survivor whose rank is not below n_rest is dropped, a survivor row
 *   nothing maps to is unspecified, nothing is written outside the T rows.  16-byte stores when every output starts on 16
 *   bytes.  1 launch.
 * assemble_backward: upstream gradients (T, w) f32, any may be NULL (zeros).  grad_coord[l] (n_l, 3) f32 and grad_attr[l]
 *   (n_l, P) of attr_dtype, the dense coarse gradients (a row is its survivor's upstream row or zero) and grad_shs_fine
 *   (n_masked, sh_dim); any may be NULL (not wanted).  1 launch. */
#define GDR_FINEHEAD_MAX_C 256
#define GDR_FINEHEAD_TILE_ROWS 64
#define GDR_FINEHEAD_SLAB_MIN 512
#define GDR_FINEHEAD_MAX_LEVELS 8
#define GDR_FINEHEAD_SCAN_CHUNK 1024      /* rows per workgroup of the scan */
#define GDR_FINEHEAD_WS_PACKED_FORWARD 0
#define GDR_FINEHEAD_WS_PACKED_BACKWARD 1
#define GDR_FINEHEAD_WS_PARTIALS 2
size_t gdr_finehead_workspace_bytes(int32_t what, int32_t dtype, int64_t rows, int32_t C, int32_t sh_dim);
int32_t gdr_finehead_backward_step(int32_t dtype, int32_t C, int32_t sh_dim);
int gdr_finehead_pack(const void* w1, int32_t w1_dtype, const void* w2, int32_t w2_dtype, int32_t C, int32_t sh_dim, int32_t backward,
                      void* packed, int32_t dtype, void* stream);
int gdr_finehead_forward(const void* x, int32_t dtype, const void* packed, const void* b1, int32_t b1_dtype, const void* b2, int32_t b2_dtype,
                         int64_t rows, int32_t C, int32_t sh_dim, void* out, int32_t out_dtype, void* stream);
int gdr_finehead_backward(const void* x, int32_t dtype, const void* packed, const void* b1, int32_t b1_dtype, int64_t rows, int32_t C,
                          int32_t sh_dim, const void* grad_out, int32_t grad_out_dtype, void* grad_x, void* workspace, size_t workspace_bytes,
                          void* stream);
int gdr_finehead_fold(const void* workspace, size_t workspace_bytes, int32_t dtype, int64_t rows, int32_t C, int32_t sh_dim, void* grad_w1,
                      int32_t grad_w1_dtype, void* grad_b1, int32_t grad_b1_dtype, void* grad_w2, int32_t grad_w2_dtype, void* grad_b2,
                      int32_t grad_b2_dtype, void* stream);
size_t gdr_finehead_scan_bytes(int64_t Nc, int64_t n_masked);      /* 0: the arguments are refused (gdr_last_error) */
int gdr_finehead_scan(const uint8_t* mask, int64_t Nc, const uint8_t* selected, int64_t n_masked, void* workspace, size_t workspace_bytes,
                      int32_t* rank_masked, int32_t* row_of_masked, int32_t* rank_rest, int32_t* masked_of_rest, int64_t* count, void* stream);
int gdr_finehead_assemble(int32_t n_levels, const void* const* coord, const void* const* attr, const int64_t* level_rows, int32_t attr_dtype,
                          int32_t sh_dim, const void* centers_coarse, const void* opacity_coarse, const void* scaling_coarse,
                          const void* rotation_coarse, int64_t Nc, const void* shs_fine, int64_t n_masked, const int32_t* row_of_masked,
                          const int32_t* masked_of_rest, int64_t n_rest, double opacity_shift, double scaling_shift, void* centers, void* shs,
                          void* opacity, void* scaling, void* rotation, void* stream);
int gdr_finehead_assemble_backward(int32_t n_levels, const int64_t* level_rows, int32_t attr_dtype, int32_t sh_dim, const void* grad_centers,
                                   const void* grad_shs, const void* grad_opacity, const void* grad_scaling, const void* grad_rotation,
                                   const int32_t* rank_masked, const int32_t* rank_rest, int64_t Nc, int64_t n_masked, int64_t n_rest,
                                   void* const* grad_coord, void* const* grad_attr, void* grad_centers_coarse, void* grad_opacity_coarse,
                                   void* grad_scaling_coarse, void* grad_rotation_coarse, void* grad_shs_fine, void* stream);

/* ---- volume conditioning of the volume transformer (csrc/volcond.hip; added in v17, backward-compatible) -------------------
 * What the reference computes between its image encoder and the first GroupAttBlock (Network.build_feat_vol, the view_embed
 * concat of Network.forward, the cond regrouping of VolTransformer.forward): the spherical-harmonics embedding of the Pluecker
 * rays, the modulated LayerNorm of the token rows, and the projected bilinear sampling of the token maps written straight into
 * the (B g^3, V bs^3, C + E) cond of the blocks.  The arithmetic is restated in the header of csrc/volcond.hip.  The caller owns
 * every buffer; all are device memory except `a`.  Every `*_dtype` is one of GDR_NORM_F16 / BF16 / F32 and the types of one call
 * are independent; the arithmetic is f32.  Refusals happen before any launch; no entry point allocates or synchronises with the
 * host.  No atomics: two runs are bitwise equal.  "rows of X" means a 16-byte aligned base and a row stride (elements) that is a
 * multiple of 8 and covers the row.
 *
 * ray_sh: rays (n, 6) dense of rays_dtype -> out (n, 32) dense f32, 16-byte aligned; silu != 0 applies SiLU.  1 launch.
 * modln_forward: rows of x (R, C), row o * x_inner + i at element o * x_outer_stride + i * x_stride (a token map read where the
 *   encoder left it; x_outer_stride a multiple of 8; x_inner >= R and x_outer_stride 0 for a plain matrix); rows of shift_scale (R, 2 C), shift in [:, :C], scale in [:, C:]; weight, bias: C dense
 *   elements, 16-byte aligned, or NULL (1 and 0); out (R, C) dense, 16-byte aligned.  C a multiple of 8 in
 *   8..GDR_NORM_MAX_CHANNELS, R below 2^31; R = 0 returns GDR_OK without a launch.  1 launch.
 * modln_backward: grad_out: rows of (R, C) of grad_dtype.  grad_x (R, C) dense of x_dtype, grad_shift_scale (R, 2 C) dense of
 *   ss_dtype, both 16-byte aligned; grad_weight, grad_bias: C elements of weight_dtype / bias_dtype.  A NULL output is not
 *   wanted and not computed.  The row statistics are recomputed.  workspace (only with grad_weight or grad_bias):
 *   gdr_volcond_modln_backward_bytes(R, C) bytes, 256-byte aligned: one partial pair per GDR_VOLCOND_SLAB_ROWS rows, folded in
 *   ascending order by the second launch.  1 launch, 2 with a parameter gradient.
 * sample_forward: rows (B V, h, w, C) dense channels-last, 16-byte aligned; points (r^3, 3) dense f32 in (d, h, w) grid order;
 *   w2cs (B V, 4, 4), ixts (B V, 3, 3) dense f32, the intrinsics of an (img_h, img_w) image; view_embed: rows of (V, E) or NULL
 *   with E = 0; cond (B g^3, V bs^3, C + E) dense, 16-byte aligned, g = n_group, bs = r / g.  keys (int64) and weights (f32), 4 B V
 *   r^3 entries each or both NULL: the tap table the backward reads.  1 launch.
 * sample_backward: grad_cond dense like cond; grad_rows like rows (written whole), grad_view_embed (V, E) dense; a NULL output is
 *   not wanted.  workspace (only with grad_rows): gdr_volcond_sample_backward_bytes(a) bytes, 256-byte aligned.
 *   gdr_serial_sort on the bits of B V h w + 1 launch, + 1 launch with grad_view_embed.
 * Envelope of sample (GDR_ERR_UNSUPPORTED beyond it): C a multiple of 8 in 8..GDR_VOLCOND_MAX_CHANNELS, E a multiple of 8 or 0,
 * h, w <= GDR_VOLCOND_MAX_SIDE, 4 B V r^3 <= GDR_VOLCOND_MAX_ENTRIES (what gdr_serial_sort takes), n_group divides r. */
#define GDR_VOLCOND_SLAB_ROWS 32
#define GDR_VOLCOND_MAX_CHANNELS 4096
#define GDR_VOLCOND_MAX_SIDE 1024
#define GDR_VOLCOND_MAX_ENTRIES (1 << 30)
typedef struct {
    int32_t B, V, h, w, C, E, r, n_group, img_h, img_w;
} gdr_volcond_sample_args;
int gdr_volcond_ray_sh(const void* rays, int32_t rays_dtype, int64_t n, int32_t silu, float* out, void* stream);
int gdr_volcond_modln_forward(const void* x, int64_t x_stride, int64_t x_inner, int64_t x_outer_stride, int32_t x_dtype,
                              const void* shift_scale, int64_t ss_stride, int32_t ss_dtype, const void* weight, int32_t weight_dtype, const void* bias, int32_t bias_dtype,
                              int64_t R, int32_t C, float eps, void* out, int32_t out_dtype, void* stream);
size_t gdr_volcond_modln_backward_bytes(int64_t R, int32_t C);   /* 0: the arguments are refused (gdr_last_error) */
int gdr_volcond_modln_backward(const void* grad_out, int64_t grad_stride, int32_t grad_dtype, const void* x, int64_t x_stride,
                               int64_t x_inner, int64_t x_outer_stride, int32_t x_dtype, const void* shift_scale, int64_t ss_stride, int32_t ss_dtype, const void* weight,
                               int32_t weight_dtype, const void* bias, int32_t bias_dtype, int64_t R, int32_t C, float eps,
                               void* workspace, size_t workspace_bytes, void* grad_x, void* grad_shift_scale, void* grad_weight,
                               void* grad_bias, void* stream);
int gdr_volcond_sample_forward(const gdr_volcond_sample_args* a, const void* rows, int32_t rows_dtype, const float* points,
                               const float* w2cs, const float* ixts, const void* view_embed, int64_t ve_stride, int32_t ve_dtype,
                               void* cond, int32_t cond_dtype, int64_t* keys, float* weights, void* stream);
size_t gdr_volcond_sample_backward_bytes(const gdr_volcond_sample_args* a);   /* 0: the arguments are refused (gdr_last_error) */
int gdr_volcond_sample_backward(const gdr_volcond_sample_args* a, const void* grad_cond, int32_t grad_dtype, const int64_t* keys,
                                const float* weights, void* workspace, size_t workspace_bytes, void* grad_rows, int32_t rows_dtype,
                                void* grad_view_embed, int32_t ve_dtype, void* stream);

/* ---- host-boundary helper: *flag |= 1 if the n_bytes (a multiple of 4; a, b 16-byte aligned) at a and b differ in any
 * 32-bit word.  Used by the Python boundary to verify that two calls of one render group were handed the same activated
 * tensors (see generativedensification_amd/viewgroup.py); one read of both buffers, no host synchronisation. */
int gdr_words_differ(const void* a, const void* b, uint64_t n_bytes, uint32_t* flag, void* stream);
/* ... for up to GDR_SAME_AS_MAX buffer pairs in one launch (v13; 4 until v15) */
int gdr_words_differ_multi(int32_t n, const void* const* a, const void* const* b, const uint64_t* n_bytes, uint32_t* flag,
                           void* stream);

/* ---- host-boundary helper: n_bytes from device memory to PINNED host memory behind the work queued on `stream`, with an
 * event the library pools (v13).  *ticket identifies the copy; gdr_host_copy_wait blocks until it has landed and releases
 * the ticket (every ticket must be waited for exactly once).  The upstream extension reads `num_rendered` back with a
 * blocking copy inside rasterize_gaussians; the Python boundary here reads the duplicate count of a device-sized call this
 * way after everything else of the call is enqueued — two C calls instead of ~20 us of tensor / event objects. */
int gdr_host_copy_begin(void* dst_pinned, const void* src_dev, uint64_t n_bytes, void* stream, void** ticket);
int gdr_host_copy_wait(void* ticket);

/* Zero-fill n_bytes of device memory behind the work queued on `stream` (v13): what the caller of the K7 entry points does to
 * the gradient records when it sets gdr_binning.grad_rec_cleared — one C call on a raw stream handle instead of a stream
 * context + tensor op per view on the Python side. */
int gdr_clear_async(void* dst, uint64_t n_bytes, void* stream);

/* ---- K10: visibility mask (upstream markVisible; unused by the reference) -------- */
int gdr_mark_visible(int32_t N, const float* means3D, const float* viewmatrix,
                     const float* projmatrix, uint8_t* present, void* stream);

/* ---- opt-in per-kernel timing (measurement aid, bench.py `roofline`) -----------------
 * When enabled every kernel launch is bracketed by two HIP events recorded on the SAME
 * stream the kernel runs on; gdr_profile_collect waits for them and returns, per kernel id
 * (0 <= id < gdr_kernel_count(), names from gdr_kernel_name), the summed elapsed ms and the
 * launch count since the last reset.  Process-wide switch; off by default (no events). */
int gdr_profile_enable(int on);
int gdr_profile_collect(double* ms_total, uint64_t* launches, int32_t n, int32_t reset);
int gdr_kernel_count(void);
const char* gdr_kernel_name(int32_t id);

#ifdef __cplusplus
}
#endif
#endif /* GDR_H */

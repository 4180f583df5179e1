// serialize.hip — point-cloud serialization for the point decoder (include/gdr.h gdr_serial_*): space-filling-curve codes
// of integer grid cells, their stable argsort with the inverse permutation, and the patch index tables of the serialized
// attention.  What the reference does with tensor ops in Point.serialization (lightning/point_decoder/utils/structure.py)
// and SerializedAttention.get_padding_and_inverse (lightning/point_decoder/autoencoder.py).
//
// Codes (depth bits per axis; x, y, z are the depth low bits of the three columns of grid_coord):
//   z              bit i of x -> bit 3i+2, of y -> 3i+1, of z -> 3i
//   hilbert        Skilling's walk on (x, y, z): bit levels from the most significant, at each level dimensions 0, 1, 2: if
//                  the dimension's bit at this level is 1 all lower bits of dimension 0 are inverted, otherwise the lower
//                  bits in which the two differ are exchanged with dimension 0; then the three words are interleaved per
//                  level (dimension 0 first) and the 3 * depth bit string is replaced by its prefix XOR from the top
//   *-trans        the same on (y, x, z)
//   with batch     code = batch << (3 * depth) | code
// The walk runs on whole words in registers (serial_bits.h): depth - 1 levels of ~10 integer instructions.
//
// Sort: least-significant-digit radix sort, 8 bits per pass, of the k code rows in shared launches (row = blockIdx.y), only
// over the caller's number of significant bits.  A pass is three launches: per-tile digit counts, one exclusive scan per row
// over the (digit, tile) matrix, and the scatter.  A tile is 1024 keys: wave w of the workgroup takes keys [256 w, 256 w + 256)
// of it in four rounds of 64.  Within a round the lanes that hold the same digit are found with eight ballots; the rank of a
// key inside its tile is (keys of earlier waves) + (earlier rounds of its wave) + (lower lanes of its round), which is the
// key's rank in memory order: every pass is stable, so equal codes end in ascending point index.  Values are 32-bit point
// indices, implicit (= position) in the first pass; the last pass writes order and inverse as int64 and no keys.
//
// Patch tables: one launch.  Every workgroup scans the segment table (B <= 1024) into LDS, then each thread finds the segment
// of its slot by binary search.  Every write is bounded by the caller's buffer sizes whatever the offsets on the device say.
#include "gdr_common.h"
#include "host_util.h"
#include "serial_bits.h"

namespace gdr {
namespace {

constexpr int SR_BLOCK = 256;
constexpr int SR_WAVES = SR_BLOCK / 64;
constexpr int SR_ROUNDS = GDR_SERIAL_SORT_TILE / SR_BLOCK;
constexpr int SR_RADIX = 256;
static_assert(SR_ROUNDS * SR_BLOCK == GDR_SERIAL_SORT_TILE, "tile = whole rounds of the workgroup");

struct EncP {
    const void* coord; const int64_t* batch; int64_t* code;
    int64_t s0, s1;
    uint32_t n; int32_t depth, k, coord64;
    int32_t ord[GDR_SERIAL_MAX_ORDERS];
};

__global__ __launch_bounds__(SR_BLOCK) void serial_encode_kernel(const EncP p) {
    const uint32_t i = blockIdx.x * SR_BLOCK + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t m = (1u << p.depth) - 1u;
    uint32_t x, y, z;
    if (p.coord64) {
        const int64_t* c = (const int64_t*)p.coord + (int64_t)i * p.s0;
        x = (uint32_t)c[0] & m; y = (uint32_t)c[p.s1] & m; z = (uint32_t)c[2 * p.s1] & m;
    } else {
        const int32_t* c = (const int32_t*)p.coord + (int64_t)i * p.s0;
        x = (uint32_t)c[0] & m; y = (uint32_t)c[p.s1] & m; z = (uint32_t)c[2 * p.s1] & m;
    }
    const uint64_t hi = p.batch ? (uint64_t)p.batch[i] << (3 * p.depth) : 0;
    unsigned need = 0;
    for (int r = 0; r < p.k; ++r) need |= 1u << p.ord[r];
    uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (need & 1u) c0 = serial_interleave3(x, y, z);
    if (need & 2u) c1 = serial_interleave3(y, x, z);
    if (need & 4u) c2 = serial_hilbert_encode(x, y, z, p.depth);
    if (need & 8u) c3 = serial_hilbert_encode(y, x, z, p.depth);
    for (int r = 0; r < p.k; ++r) {
        const int o = p.ord[r];
        const uint64_t c = o == 0 ? c0 : (o == 1 ? c1 : (o == 2 ? c2 : c3));
        p.code[(size_t)r * p.n + i] = (int64_t)(hi | c);
    }
}

__global__ __launch_bounds__(SR_BLOCK) void serial_decode_kernel(const int64_t* __restrict__ code, uint32_t n, int depth,
                                                                 int hilbert, int64_t* __restrict__ grid,
                                                                 int64_t* __restrict__ batch) {
    const uint32_t i = blockIdx.x * SR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t c = code[i];
    const uint64_t low = (uint64_t)c & ((UINT64_C(1) << (3 * depth)) - 1);
    uint32_t x, y, z;
    if (hilbert) serial_hilbert_decode(low, depth, &x, &y, &z);
    else { x = serial_compact3(low >> 2); y = serial_compact3(low >> 1); z = serial_compact3(low); }
    grid[(size_t)i * 3 + 0] = x; grid[(size_t)i * 3 + 1] = y; grid[(size_t)i * 3 + 2] = z;
    batch[i] = c >> (3 * depth);
}

struct SortP {
    const uint64_t* kin; const uint32_t* vin;    // (k, n); vin NULL: the value of a key is its position
    uint64_t* kout; uint32_t* vout;              // (k, n); unused in the last pass
    int64_t* order; int64_t* inverse;            // (k, n); the last pass only (order != NULL)
    uint32_t* hist;                              // (k, 256, nblk)
    uint32_t n, nblk; int32_t shift; uint32_t mask;
};

// hist[row][digit][tile] = keys of the tile with that digit
__global__ __launch_bounds__(SR_BLOCK) void serial_hist_kernel(const SortP p) {
    __shared__ uint32_t cnt[SR_RADIX];
    const uint32_t row = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    cnt[tid] = 0;
    __syncthreads();
    const uint64_t* kin = p.kin + (size_t)row * p.n;
    for (int r = 0; r < SR_ROUNDS; ++r) {
        const uint32_t idx = blk * GDR_SERIAL_SORT_TILE + r * SR_BLOCK + tid;
        if (idx < p.n) atomicAdd(&cnt[(uint32_t)(kin[idx] >> p.shift) & p.mask], 1u);
    }
    __syncthreads();
    p.hist[((size_t)row * SR_RADIX + tid) * p.nblk + blk] = cnt[tid];
}

// exclusive scan of one row's (digit, tile) matrix in digit-major order, in place: one workgroup per row, thread = digit
__global__ __launch_bounds__(SR_BLOCK) void serial_scan_kernel(uint32_t* __restrict__ hist, uint32_t nblk) {
    __shared__ uint32_t tot[SR_RADIX];
    const uint32_t tid = threadIdx.x;
    uint32_t* h = hist + ((size_t)blockIdx.x * SR_RADIX + tid) * nblk;
    uint32_t sum = 0;
    for (uint32_t b = 0; b < nblk; ++b) sum += h[b];
    tot[tid] = sum;
    __syncthreads();
    for (int off = 1; off < SR_RADIX; off <<= 1) {
        const uint32_t add = tid >= (uint32_t)off ? tot[tid - off] : 0;
        __syncthreads();
        tot[tid] += add;
        __syncthreads();
    }
    uint32_t base = tot[tid] - sum;
    for (uint32_t b = 0; b < nblk; ++b) {
        const uint32_t t = h[b];
        h[b] = base;
        base += t;
    }
}

__global__ __launch_bounds__(SR_BLOCK) void serial_scatter_kernel(const SortP p) {
    __shared__ uint32_t cnt[SR_WAVES][SR_RADIX];
    const uint32_t row = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63u;
    for (int i = 0; i < SR_WAVES; ++i) cnt[i][tid] = 0;
    __syncthreads();
    const uint64_t* kin = p.kin + (size_t)row * p.n;
    uint64_t key[SR_ROUNDS];
    uint32_t val[SR_ROUNDS], pos[SR_ROUNDS], dig[SR_ROUNDS];
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; ++r) {
        const uint32_t idx = blk * GDR_SERIAL_SORT_TILE + (w * SR_ROUNDS + r) * 64u + lane;
        const bool valid = idx < p.n;
        key[r] = valid ? kin[idx] : 0;
        val[r] = valid ? (p.vin ? p.vin[(size_t)row * p.n + idx] : idx) : 0xffffffffu;
        const uint32_t d = (uint32_t)(key[r] >> p.shift) & p.mask;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long mb = __ballot(bit);
            peers &= bit ? mb : ~mb;
        }
        const uint32_t rank = __popcll(peers & ((1ull << lane) - 1ull));
        const uint32_t prior = cnt[w][d];
        __syncthreads();
        if (valid && rank == 0) cnt[w][d] = prior + (uint32_t)__popcll(peers);
        __syncthreads();
        pos[r] = prior + rank;
        dig[r] = d;
    }
    {   // per digit: the tile's base in the output, then the waves of the tile in order
        uint32_t g = p.hist[((size_t)row * SR_RADIX + tid) * p.nblk + blk];
        for (int i = 0; i < SR_WAVES; ++i) {
            const uint32_t t = cnt[i][tid];
            cnt[i][tid] = g;
            g += t;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SR_ROUNDS; ++r) {
        const uint32_t dst = cnt[w][dig[r]] + pos[r];
        if (val[r] == 0xffffffffu || dst >= p.n) continue;
        if (p.order) {
            p.order[(size_t)row * p.n + dst] = val[r];
            if (val[r] < p.n) p.inverse[(size_t)row * p.n + val[r]] = dst;
        } else {
            p.kout[(size_t)row * p.n + dst] = key[r];
            p.vout[(size_t)row * p.n + dst] = val[r];
        }
    }
}

// first index in [0, n) whose value exceeds v (n if none): tab is non-decreasing
__device__ __forceinline__ int upper_bound_lds(const int64_t* tab, int n, int64_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct PatchP {
    const int64_t* offset;    // B segment ends (off_1 .. off_B; off_0 = 0)
    int64_t* pad; int64_t* unpad; int32_t* cu;
    int64_t n, total;         // sizes of unpad / pad
    int32_t B, P, n_seq;      // cu has n_seq + 1 entries
};

__global__ __launch_bounds__(SR_BLOCK) void serial_patch_kernel(const PatchP p) {
    // starts of the segments in the point, padded-slot and sequence numbering (entry B: the totals)
    __shared__ int64_t off[GDR_SERIAL_MAX_SEGMENTS + 1], poff[GDR_SERIAL_MAX_SEGMENTS + 1], soff[GDR_SERIAL_MAX_SEGMENTS + 1];
    __shared__ int64_t part_m[SR_BLOCK], part_s[SR_BLOCK];
    const int tid = threadIdx.x, B = p.B, P = p.P;
    const int chunk = (B + SR_BLOCK - 1) / SR_BLOCK, lo = tid * chunk, hi = min(B, lo + chunk);
    int64_t sm = 0, ss = 0;
    for (int i = lo; i < hi; ++i) {
        const int64_t a = i ? p.offset[i - 1] : 0, n = max(p.offset[i] - a, (int64_t)0);
        sm += n <= P ? n : (n + P - 1) / P * P;
        ss += n == 0 ? 0 : (n <= P ? 1 : (n + P - 1) / P);
    }
    part_m[tid] = sm; part_s[tid] = ss;
    __syncthreads();
    int64_t bm = 0, bs = 0;
    for (int t = 0; t < tid; ++t) { bm += part_m[t]; bs += part_s[t]; }
    for (int i = lo; i < hi; ++i) {
        const int64_t a = i ? p.offset[i - 1] : 0, n = max(p.offset[i] - a, (int64_t)0);
        off[i] = a; poff[i] = bm; soff[i] = bs;
        bm += n <= P ? n : (n + P - 1) / P * P;
        bs += n == 0 ? 0 : (n <= P ? 1 : (n + P - 1) / P);
        if (i == B - 1) { off[B] = a + n; poff[B] = bm; soff[B] = bs; }
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * SR_BLOCK, first = (int64_t)blockIdx.x * SR_BLOCK + tid;
    for (int64_t t = first; t < p.total; t += stride) {         // pad: padded slot -> point
        const int i = upper_bound_lds(poff, B + 1, t) - 1;
        if (i < 0 || i >= B) continue;
        const int64_t l = t - poff[i], n = off[i + 1] - off[i];
        p.pad[t] = off[i] + (l < n ? l : l - P);
    }
    for (int64_t j = first; j < p.n; j += stride) {             // unpad: point -> padded slot
        const int i = upper_bound_lds(off, B + 1, j) - 1;
        if (i < 0 || i >= B) continue;
        p.unpad[j] = j + poff[i] - off[i];
    }
    for (int64_t s = first; s <= p.n_seq; s += stride) {        // cu_seqlens: sequence -> first padded slot
        const int i = upper_bound_lds(soff, B + 1, s) - 1;
        p.cu[s] = (int32_t)((i < 0 || i >= B) ? poff[B] : poff[i] + (s - soff[i]) * P);
    }
}

const char* serial_check(int64_t N, int32_t depth) {
    if (N < 0 || N > GDR_SERIAL_MAX_POINTS) return "serial: N must be in 0..GDR_SERIAL_MAX_POINTS";
    if (depth < 1 || depth > GDR_SERIAL_MAX_DEPTH) return "serial: depth must be in 1..16";
    return nullptr;
}

struct SortWs { size_t keys[2], vals[2], hist, bytes; };

SortWs sort_workspace(int32_t k, int64_t N) {
    SortWs w;
    const size_t kn = (size_t)k * (size_t)N, nblk = ((size_t)N + GDR_SERIAL_SORT_TILE - 1) / GDR_SERIAL_SORT_TILE;
    size_t at = 0;
    for (int i = 0; i < 2; ++i) { w.keys[i] = at; at += align_up(kn * 8); }
    for (int i = 0; i < 2; ++i) { w.vals[i] = at; at += align_up(kn * 4); }
    w.hist = at; at += align_up((size_t)k * SR_RADIX * nblk * 4);
    w.bytes = at;
    return w;
}

}  // namespace
}  // namespace gdr

using namespace gdr;

extern "C" {

int gdr_serial_encode(const void* grid_coord, const int64_t* strides, int32_t coord_is_int64, const int64_t* batch, int64_t N,
                      int32_t depth, int32_t k, const int32_t* orders, int64_t* code, void* stream) {
    if (const char* why = serial_check(N, depth)) return invalid_arg(why);
    if (k < 1 || k > GDR_SERIAL_MAX_ORDERS || !orders) return invalid_arg("serial_encode: k must be in 1..GDR_SERIAL_MAX_ORDERS");
    if (!strides) return invalid_arg("serial_encode: NULL strides");
    EncP p = {};
    for (int r = 0; r < k; ++r) {
        if (orders[r] < GDR_SERIAL_Z || orders[r] > GDR_SERIAL_HILBERT_TRANS) return invalid_arg("serial_encode: unknown order");
        p.ord[r] = orders[r];
    }
    if (N == 0) return GDR_OK;
    if (!grid_coord || !code) return invalid_arg("serial_encode: NULL argument");
    if (misaligned(grid_coord, coord_is_int64 ? 7 : 3) || misaligned(code, 7) || misaligned(batch, 7))
        return invalid_arg("serial_encode: unaligned buffer");
    p.coord = grid_coord; p.batch = batch; p.code = code; p.s0 = strides[0]; p.s1 = strides[1];
    p.n = (uint32_t)N; p.depth = depth; p.k = k; p.coord64 = coord_is_int64 ? 1 : 0;
    hipLaunchKernelGGL(serial_encode_kernel, dim3(div_up(N, SR_BLOCK)), dim3(SR_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("serial_encode_kernel");
}

int gdr_serial_decode(const int64_t* code, int64_t N, int32_t depth, int32_t order, int64_t* grid_coord, int64_t* batch,
                      void* stream) {
    if (const char* why = serial_check(N, depth)) return invalid_arg(why);
    if (order != GDR_SERIAL_Z && order != GDR_SERIAL_HILBERT) return invalid_arg("serial_decode: order must be z or hilbert");
    if (N == 0) return GDR_OK;
    if (!code || !grid_coord || !batch) return invalid_arg("serial_decode: NULL argument");
    if (misaligned(code, 7) || misaligned(grid_coord, 7) || misaligned(batch, 7))
        return invalid_arg("serial_decode: unaligned buffer");
    hipLaunchKernelGGL(serial_decode_kernel, dim3(div_up(N, SR_BLOCK)), dim3(SR_BLOCK), 0, (hipStream_t)stream, code,
                       (uint32_t)N, depth, order == GDR_SERIAL_HILBERT ? 1 : 0, grid_coord, batch);
    return launch_status("serial_decode_kernel");
}

size_t gdr_serial_sort_bytes(int32_t k, int64_t N) {
    if (k < 1 || k > GDR_SERIAL_MAX_ORDERS || N < 0 || N > GDR_SERIAL_MAX_POINTS) {
        invalid_arg("serial_sort_bytes: k or N outside the envelope");
        return 0;
    }
    return sort_workspace(k, N).bytes + 256;   // (never 0 for valid arguments)
}

int gdr_serial_sort(const int64_t* code, int32_t k, int64_t N, int32_t bits, void* workspace, size_t workspace_bytes,
                    int64_t* order, int64_t* inverse, void* stream) {
    if (k < 1 || k > GDR_SERIAL_MAX_ORDERS) return invalid_arg("serial_sort: k must be in 1..GDR_SERIAL_MAX_ORDERS");
    if (N < 0 || N > GDR_SERIAL_MAX_POINTS) return invalid_arg("serial_sort: N must be in 0..GDR_SERIAL_MAX_POINTS");
    if (bits < 1 || bits > 63) return invalid_arg("serial_sort: bits must be in 1..63");
    if (N == 0) return GDR_OK;
    if (!code || !order || !inverse || !workspace) return invalid_arg("serial_sort: NULL argument");
    if (misaligned(code, 7) || misaligned(order, 7) || misaligned(inverse, 7) || misaligned(workspace, 255))
        return invalid_arg("serial_sort: unaligned buffer");
    const SortWs ws = sort_workspace(k, N);
    if (workspace_bytes < ws.bytes)
        return workspace_too_small("serial_sort: workspace smaller than gdr_serial_sort_bytes");
    char* base = (char*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t nblk = (uint32_t)div_up(N, GDR_SERIAL_SORT_TILE);
    const dim3 grid(nblk, k);
    const int passes = (bits + 7) / 8;
    SortP p = {};
    p.hist = (uint32_t*)(base + ws.hist); p.n = (uint32_t)N; p.nblk = nblk;
    p.kin = (const uint64_t*)code; p.vin = nullptr;
    for (int pass = 0; pass < passes; ++pass) {
        const int width = bits - 8 * pass < 8 ? bits - 8 * pass : 8;
        p.shift = 8 * pass; p.mask = (1u << width) - 1u;
        const bool last = pass == passes - 1;
        p.kout = (uint64_t*)(base + ws.keys[pass & 1]); p.vout = (uint32_t*)(base + ws.vals[pass & 1]);
        p.order = last ? order : nullptr; p.inverse = last ? inverse : nullptr;
        hipLaunchKernelGGL(serial_hist_kernel, grid, dim3(SR_BLOCK), 0, st, p);
        hipLaunchKernelGGL(serial_scan_kernel, dim3(k), dim3(SR_BLOCK), 0, st, p.hist, nblk);
        hipLaunchKernelGGL(serial_scatter_kernel, grid, dim3(SR_BLOCK), 0, st, p);
        p.kin = p.kout; p.vin = p.vout;
    }
    return launch_status("serial_sort kernels");
}

int gdr_serial_patch_tables(const int64_t* offset, int32_t B, int32_t P, int64_t N, int64_t total, int32_t n_seq, int64_t* pad,
                            int64_t* unpad, int32_t* cu_seqlens, void* stream) {
    if (B < 1 || B > GDR_SERIAL_MAX_SEGMENTS) return invalid_arg("serial_patch_tables: B must be in 1..GDR_SERIAL_MAX_SEGMENTS");
    if (P < 1) return invalid_arg("serial_patch_tables: patch size must be >= 1");
    if (N < 0 || total < N || n_seq < 0 || total > INT64_C(0x7fffffff))
        return invalid_arg("serial_patch_tables: sizes must satisfy 0 <= N <= total < 2^31, n_seq >= 0");
    if (!offset || !cu_seqlens || (N && !unpad) || (total && !pad)) return invalid_arg("serial_patch_tables: NULL argument");
    if (misaligned(offset, 7) || misaligned(pad, 7) || misaligned(unpad, 7) || misaligned(cu_seqlens, 3))
        return invalid_arg("serial_patch_tables: unaligned buffer");
    PatchP p = {};
    p.offset = offset; p.pad = pad; p.unpad = unpad; p.cu = cu_seqlens; p.n = N; p.total = total; p.B = B; p.P = P; p.n_seq = n_seq;
    int64_t work = total > (int64_t)n_seq + 1 ? total : (int64_t)n_seq + 1;
    int blocks = div_up(work, SR_BLOCK * 4);    // every workgroup repeats the segment scan: a few slots per thread
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(serial_patch_kernel, dim3(blocks), dim3(SR_BLOCK), 0, (hipStream_t)stream, p);
    return launch_status("serial_patch_kernel");
}

}  // extern "C"

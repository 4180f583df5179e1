// proj_taps.h — a point projected into a camera and the four bilinear neighbours of the projected position (internal; include
// after gdr_common.h).  pointfeat.hip uses all of it.  volcond.hip, which samples at the pixel rescaled to a token map, takes
// make_taps and the bound from here and writes the projection out (its project_taps says why).
//   q = R p + t (w2c[v][:3,:3], w2c[v][:3,3]);  h = K q;  x = h0 / h2, y = h1 / h2, z = h2.
// A (point, view) pair is degenerate when h2 == 0 or x or y is not finite or lies outside +-2^30: it carries x = y = 0 and
// ok = false, and none of its neighbours counts as inside.  h2 < 0 is not degenerate: it projects mirrored.
#pragma once

namespace gdr {
namespace {      // the including file's own names, as in ln_rows.h (device_math.h has another Cam / load_cam for the render path)

constexpr float PT_MAX_POS = 1073741824.f;   // 2^30: positions up to here floor exactly into an int

struct Cam { float r[9], t[3], k[9]; };

__device__ __forceinline__ Cam load_cam(const float* __restrict__ w2c, const float* __restrict__ ixt, int64_t v) {
    Cam c;
    const float* m = w2c + v * 16;
    const float* k = ixt + v * 9;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) { c.r[i * 3 + j] = m[i * 4 + j]; c.k[i * 3 + j] = k[i * 3 + j]; }
        c.t[i] = m[i * 4 + 3];
    }
    return c;
}

struct Proj { float x, y, z; bool ok; };

__device__ __forceinline__ Proj project(const Cam& c, float px, float py, float pz) {
    const float q0 = c.r[0] * px + c.r[1] * py + c.r[2] * pz + c.t[0];
    const float q1 = c.r[3] * px + c.r[4] * py + c.r[5] * pz + c.t[1];
    const float q2 = c.r[6] * px + c.r[7] * py + c.r[8] * pz + c.t[2];
    const float h0 = c.k[0] * q0 + c.k[1] * q1 + c.k[2] * q2;
    const float h1 = c.k[3] * q0 + c.k[4] * q1 + c.k[5] * q2;
    const float h2 = c.k[6] * q0 + c.k[7] * q1 + c.k[8] * q2;
    Proj o;
    o.z = h2;
    o.ok = h2 != 0.f;
    o.x = o.ok ? h0 / h2 : 0.f;
    o.y = o.ok ? h1 / h2 : 0.f;
    o.ok = o.ok && fabsf(o.x) <= PT_MAX_POS && fabsf(o.y) <= PT_MAX_POS;     // (false for NaN and inf)
    if (!o.ok) o.x = o.y = 0.f;       // a degenerate pair carries finite weights (its neighbours all count as outside)
    return o;
}

// (gx, gy, gz) at (x, y, z) -> added to the point gradient.  A degenerate pair arrives with gx = gy = 0.
__device__ __forceinline__ void project_bwd(const Cam& c, const Proj& p, float gx, float gy, float gz, float& dx, float& dy,
                                            float& dz) {
    float dh0 = 0.f, dh1 = 0.f, dh2 = gz;
    if (p.ok) {
        dh0 = gx / p.z;
        dh1 = gy / p.z;
        dh2 -= (gx * p.x + gy * p.y) / p.z;
    }
    const float dq0 = c.k[0] * dh0 + c.k[3] * dh1 + c.k[6] * dh2;
    const float dq1 = c.k[1] * dh0 + c.k[4] * dh1 + c.k[7] * dh2;
    const float dq2 = c.k[2] * dh0 + c.k[5] * dh1 + c.k[8] * dh2;
    dx += c.r[0] * dq0 + c.r[3] * dq1 + c.r[6] * dq2;
    dy += c.r[1] * dq0 + c.r[4] * dq1 + c.r[7] * dq2;
    dz += c.r[2] * dq0 + c.r[5] * dq1 + c.r[8] * dq2;
}

// The four neighbours of a position in an (H, W) map: texel coordinates clamped into the map (every address formed from them is
// valid), `in` says which neighbours really lie inside, w their weights.  Index t = 2 * (y neighbour) + (x neighbour).
struct Taps { int xc[2], yc[2]; float wx[2], wy[2]; bool in[4]; };

__device__ __forceinline__ Taps make_taps(const Proj& p, int H, int W) {
    Taps t;
    const float xf = p.ok ? floorf(p.x) : 0.f, yf = p.ok ? floorf(p.y) : 0.f;
    const int x0 = (int)xf, y0 = (int)yf;          // |x|, |y| <= 2^30: exact, and x0 + 1 cannot overflow
    t.wx[1] = p.x - xf; t.wx[0] = (xf + 1.f) - p.x;
    t.wy[1] = p.y - yf; t.wy[0] = (yf + 1.f) - p.y;
    bool xin[2], yin[2];
    for (int i = 0; i < 2; ++i) {
        xin[i] = p.ok && x0 + i >= 0 && x0 + i < W;
        yin[i] = p.ok && y0 + i >= 0 && y0 + i < H;
        t.xc[i] = min(max(x0 + i, 0), W - 1);
        t.yc[i] = min(max(y0 + i, 0), H - 1);
    }
    for (int i = 0; i < 4; ++i) t.in[i] = yin[i >> 1] && xin[i & 1];
    return t;
}

}  // namespace
}  // namespace gdr

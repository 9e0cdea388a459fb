// Primitive set-up of the z-buffer rasteriser (render.hip), host and device,
// header only: everything between a world-space primitive and the integers the
// raster loops work on.  tests/render_ref.py is the definition; this file
// restates it operation for operation, and tests/cpp/render_setup_test.cpp runs
// it on the host against that file.
//
//   to_camera       p_cam = R^T (p - t), f64, sums left to right
//   clip_polygon    Sutherland-Hodgman in camera space against, in this order,
//                   near, far, left, right, top, bottom; the four side planes
//                   are widened by the guard band kGuard pixels.  A vertex
//                   with distance >= 0 is inside.  A new vertex is always
//                   I + t (O - I), t = dI / (dI - dO), from the inside vertex I
//                   to the outside vertex O, so both triangles at a shared
//                   edge get the same point.  Colours are carried as f64 and
//                   rounded half up to u8 once, after the last plane.
//   project         u = fx X / Z + cx, v = fy Y / Z + cy, 1/Z; triangles snap to
//                   1/16 pixel (floor(16 u + 0.5)), lines and points to the pixel
//                   that contains the projection (floor(u)).  Pixel centres sit
//                   at (i + 1/2, j + 1/2), i.e. at 16 i + 8 in fixed point.
//   fan             polygon v0 .. vn-1 -> triangles (v0, vi, vi+1)
//   tri_prepare     winding normalised by swapping vertices 1 and 2, bounding
//                   box of covered pixel centres cut to the viewport
//   tri_pixel       int64 edge functions with the top-left rule, the exact
//                   integer Gouraud blend (round half up) and 1/Z
//   line_*          the midpoint (Bresenham) walk in closed form, from the
//                   endpoint lower in (y, x)
//
// Fixed-point bounds.  The viewport is at most kMaxDim = 8192 pixels per axis and
// the guard band kGuard = 32768 pixels, so a snapped coordinate is at most
// (8192 + 32768) * 16 + 16 < 2^20 in magnitude (checked: a primitive that
// exceeds it, which only non-finite arithmetic produces, is skipped and
// counted).  A coordinate difference is below 2^21, an edge function (two
// products of two differences) below 2^43, and the colour numerator
// 2 * 255 * 2^43 + 2^43 below 2^53: every integer fits int64 and converts to f64
// exactly.
//
// Build with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RENDER_HD __host__ __device__
#else
#define RENDER_HD
#endif

namespace render_setup {

constexpr int kMaxDim = 8192;          // viewport limit per axis
constexpr double kGuard = 32768.0;     // guard band around the viewport, pixels
constexpr int kSubBits = 4;            // 1/16 pixel
constexpr int kMaxPoly = 9;            // a triangle cut by six planes
constexpr double kSnapLimit = (kMaxDim + kGuard) * 16.0 + 16.0;
constexpr double kPixelLimit = kMaxDim + kGuard + 1.0;
constexpr int kMaxPointSize = 7;
enum Kind { kPoint = 0, kLine = 1, kTriangle = 2 };     // a lower kind wins a depth tie
constexpr int kIndexBits = 30;
constexpr uint64_t kEmptyKey = ~0ull;

struct Camera {
    double fx, fy, cx, cy, znear, zfar;
    double kl, kr, kt, kb;             // cx + G, (w + G) - cx, cy + G, (h + G) - cy
    int w, h;
};

struct Vert {
    double x, y, z;
    double c[3];
};

// the clipped polygon of one triangle on the screen
struct ScreenPoly {
    int n;
    int32_t x[kMaxPoly], y[kMaxPoly];  // 1/16 pixel
    double iz[kMaxPoly];
    uint8_t c[kMaxPoly][3];
};

struct ScreenTri {
    int32_t x[3], y[3];
    double iz[3];
    uint8_t c[3][3];
    int64_t area2;                     // > 0 after tri_prepare
    int32_t bx0, by0, bx1, by1;        // pixels whose centre can be covered, inclusive, inside the viewport
};

struct ScreenLine {
    int32_t x0, y0, x1, y1;            // pixels; (y0, x0) <= (y1, x1)
    double iz0, iz1;
    int32_t n;                         // steps along the major axis
    int32_t dminor;                    // |delta| along the minor axis
    int32_t sx;                        // sign of x1 - x0 (+1 when equal)
    int32_t xmajor;
    int32_t k0, k1;                    // the steps whose major coordinate is inside the viewport (k0 > k1: none)
};

RENDER_HD inline bool camera_valid(const double cam[6], int w, int h)
{
    for (int i = 0; i < 6; i++)
        if (!std::isfinite(cam[i])) return false;
    if (w < 1 || w > kMaxDim || h < 1 || h > kMaxDim) return false;
    if (cam[0] == 0.0 || cam[1] == 0.0) return false;
    return cam[4] > 0.0 && cam[4] < cam[5];
}

RENDER_HD inline Camera make_camera(const double cam[6], int w, int h)
{
    Camera c;
    c.fx = cam[0]; c.fy = cam[1]; c.cx = cam[2]; c.cy = cam[3]; c.znear = cam[4]; c.zfar = cam[5];
    c.kl = c.cx + kGuard;
    c.kr = ((double)w + kGuard) - c.cx;
    c.kt = c.cy + kGuard;
    c.kb = ((double)h + kGuard) - c.cy;
    c.w = w; c.h = h;
    return c;
}

RENDER_HD inline bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// view: R (3 x 3, row major, camera to world) then t
RENDER_HD inline void to_camera(const double* view, const float* p, double* out)
{
    const double d0 = (double)p[0] - view[9], d1 = (double)p[1] - view[10], d2 = (double)p[2] - view[11];
    out[0] = (view[0] * d0 + view[3] * d1) + view[6] * d2;
    out[1] = (view[1] * d0 + view[4] * d1) + view[7] * d2;
    out[2] = (view[2] * d0 + view[5] * d1) + view[8] * d2;
}

RENDER_HD inline double plane_dist(const Camera& c, int k, double x, double y, double z)
{
    switch (k) {
    case 0: return z - c.znear;
    case 1: return c.zfar - z;
    case 2: return c.fx * x + c.kl * z;
    case 3: return c.kr * z - c.fx * x;
    case 4: return c.fy * y + c.kt * z;
    default: return c.kb * z - c.fy * y;
    }
}

// the point of the edge from the inside vertex a (distance da >= 0) to the outside vertex b (db < 0)
RENDER_HD inline Vert clip_point(const Vert& a, double da, const Vert& b, double db)
{
    const double t = da / (da - db);
    Vert r;
    r.x = a.x + t * (b.x - a.x);
    r.y = a.y + t * (b.y - a.y);
    r.z = a.z + t * (b.z - a.z);
    for (int i = 0; i < 3; i++) r.c[i] = a.c[i] + t * (b.c[i] - a.c[i]);
    return r;
}

// p: n vertices, room for kMaxPoly; returns the new count (0: nothing left)
RENDER_HD inline int clip_polygon(const Camera& c, Vert* p, int n)
{
    Vert q[kMaxPoly];
    double d[kMaxPoly];
    for (int k = 0; k < 6; k++) {
        bool any_in = false, any_out = false;
        for (int i = 0; i < n; i++) {
            d[i] = plane_dist(c, k, p[i].x, p[i].y, p[i].z);
            if (d[i] >= 0.0) any_in = true;
            else any_out = true;
        }
        if (!any_out) continue;
        if (!any_in) return 0;
        int m = 0;
        for (int i = 0; i < n; i++) {
            const int j = i == 0 ? n - 1 : i - 1;          // the edge j -> i
            const bool in_i = d[i] >= 0.0, in_j = d[j] >= 0.0;
            if (in_i) {
                if (!in_j && m < kMaxPoly) q[m++] = clip_point(p[i], d[i], p[j], d[j]);
                if (m < kMaxPoly) q[m++] = p[i];
            } else if (in_j) {
                if (m < kMaxPoly) q[m++] = clip_point(p[j], d[j], p[i], d[i]);
            }
        }
        for (int i = 0; i < m; i++) p[i] = q[i];
        n = m;
        if (n < 3) return 0;
    }
    return n;
}

RENDER_HD inline uint8_t round_color(double v)
{
    const double r = std::floor(v + 0.5);
    if (!(r > 0.0)) return 0;
    return r >= 255.0 ? (uint8_t)255 : (uint8_t)r;
}

// the clipped, snapped polygon of the triangle p0 p1 p2 (world space, finite) with colours c0 c1 c2.
// Returns the vertex count (0: clipped away), or -1 when a coordinate leaves the fixed-point range.
RENDER_HD inline int setup_triangle(const Camera& cam, const double* view, const float* p0, const float* p1,
                                    const float* p2, const uint8_t* c0, const uint8_t* c1, const uint8_t* c2,
                                    ScreenPoly* out)
{
    Vert v[kMaxPoly];
    const float* p[3] = {p0, p1, p2};
    const uint8_t* col[3] = {c0, c1, c2};
    for (int i = 0; i < 3; i++) {
        double q[3];
        to_camera(view, p[i], q);
        v[i].x = q[0]; v[i].y = q[1]; v[i].z = q[2];
        for (int k = 0; k < 3; k++) v[i].c[k] = (double)col[i][k];
    }
    const int n = clip_polygon(cam, v, 3);
    out->n = 0;
    if (n == 0) return 0;
    for (int i = 0; i < n; i++) {
        const double u = (cam.fx * v[i].x) / v[i].z + cam.cx;
        const double w = (cam.fy * v[i].y) / v[i].z + cam.cy;
        const double su = std::floor(u * 16.0 + 0.5), sv = std::floor(w * 16.0 + 0.5);
        if (!(su >= -kSnapLimit && su <= kSnapLimit && sv >= -kSnapLimit && sv <= kSnapLimit)) return -1;
        out->x[i] = (int32_t)su;
        out->y[i] = (int32_t)sv;
        out->iz[i] = 1.0 / v[i].z;
        for (int k = 0; k < 3; k++) out->c[i][k] = round_color(v[i].c[k]);
    }
    out->n = n;
    return n;
}

RENDER_HD inline int fan_count(int n) { return n < 3 ? 0 : n - 2; }

// piece i (0 .. fan_count - 1) of the polygon, prepared; false: it covers nothing
RENDER_HD inline bool tri_prepare(const Camera& cam, const ScreenPoly& poly, int piece, ScreenTri* t)
{
    const int idx[3] = {0, piece + 1, piece + 2};
    for (int i = 0; i < 3; i++) {
        t->x[i] = poly.x[idx[i]];
        t->y[i] = poly.y[idx[i]];
        t->iz[i] = poly.iz[idx[i]];
        for (int k = 0; k < 3; k++) t->c[i][k] = poly.c[idx[i]][k];
    }
    int64_t a = (int64_t)(t->x[1] - t->x[0]) * (int64_t)(t->y[2] - t->y[0]) -
                (int64_t)(t->y[1] - t->y[0]) * (int64_t)(t->x[2] - t->x[0]);
    if (a == 0) return false;
    if (a < 0) {
        a = -a;
        const int32_t tx = t->x[1], ty = t->y[1];
        t->x[1] = t->x[2]; t->y[1] = t->y[2];
        t->x[2] = tx; t->y[2] = ty;
        const double tz = t->iz[1];
        t->iz[1] = t->iz[2];
        t->iz[2] = tz;
        for (int k = 0; k < 3; k++) {
            const uint8_t tc = t->c[1][k];
            t->c[1][k] = t->c[2][k];
            t->c[2][k] = tc;
        }
    }
    t->area2 = a;
    int32_t minx = t->x[0], maxx = t->x[0], miny = t->y[0], maxy = t->y[0];
    for (int i = 1; i < 3; i++) {
        minx = t->x[i] < minx ? t->x[i] : minx;
        maxx = t->x[i] > maxx ? t->x[i] : maxx;
        miny = t->y[i] < miny ? t->y[i] : miny;
        maxy = t->y[i] > maxy ? t->y[i] : maxy;
    }
    // centres 16 i + 8 in [min, max]: i >= ceil((min - 8) / 16), i <= floor((max - 8) / 16)
    int32_t bx0 = (minx + 7) >> kSubBits, bx1 = (maxx - 8) >> kSubBits;
    int32_t by0 = (miny + 7) >> kSubBits, by1 = (maxy - 8) >> kSubBits;
    if (bx0 < 0) bx0 = 0;
    if (by0 < 0) by0 = 0;
    if (bx1 > cam.w - 1) bx1 = cam.w - 1;
    if (by1 > cam.h - 1) by1 = cam.h - 1;
    t->bx0 = bx0; t->by0 = by0; t->bx1 = bx1; t->by1 = by1;
    return bx0 <= bx1 && by0 <= by1;
}

// edge a -> b at the point (px, py), all in 1/16 pixel
RENDER_HD inline int64_t edge_fn(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py)
{
    return (int64_t)(bx - ax) * (int64_t)(py - ay) - (int64_t)(by - ay) * (int64_t)(px - ax);
}

// 0 for a top or left edge (a pixel centre on it is covered), else -1
RENDER_HD inline int64_t edge_bias(int32_t ax, int32_t ay, int32_t bx, int32_t by)
{
    const int32_t dx = bx - ax, dy = by - ay;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
}

// the three edge values of the pixel centre (px, py): w[i] weighs vertex i; true when covered
RENDER_HD inline bool tri_cover(const ScreenTri& t, int px, int py, int64_t* w)
{
    const int32_t sx = px * 16 + 8, sy = py * 16 + 8;
    w[0] = edge_fn(t.x[1], t.y[1], t.x[2], t.y[2], sx, sy);
    w[1] = edge_fn(t.x[2], t.y[2], t.x[0], t.y[0], sx, sy);
    w[2] = edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], sx, sy);
    return w[0] + edge_bias(t.x[1], t.y[1], t.x[2], t.y[2]) >= 0 &&
           w[1] + edge_bias(t.x[2], t.y[2], t.x[0], t.y[0]) >= 0 &&
           w[2] + edge_bias(t.x[0], t.y[0], t.x[1], t.y[1]) >= 0;
}

RENDER_HD inline float tri_depth(const ScreenTri& t, const int64_t* w)
{
    return (float)((((double)w[0] * t.iz[0] + (double)w[1] * t.iz[1]) + (double)w[2] * t.iz[2]) / (double)t.area2);
}

RENDER_HD inline void tri_color(const ScreenTri& t, const int64_t* w, uint8_t* bgr)
{
    for (int k = 0; k < 3; k++) {
        const int64_t num = w[0] * t.c[0][k] + w[1] * t.c[1][k] + w[2] * t.c[2][k];
        bgr[k] = (uint8_t)((2 * num + t.area2) / (2 * t.area2));
    }
}

// the projection of a camera-space point as the pixel that contains it; false: outside the range
RENDER_HD inline bool project_pixel(const Camera& cam, const double* q, int32_t* px, int32_t* py)
{
    const double u = std::floor((cam.fx * q[0]) / q[2] + cam.cx), v = std::floor((cam.fy * q[1]) / q[2] + cam.cy);
    if (!(u >= -kPixelLimit && u <= kPixelLimit && v >= -kPixelLimit && v <= kPixelLimit)) return false;
    *px = (int32_t)u;
    *py = (int32_t)v;
    return true;
}

// the segment a b (world space, finite).  1: *out is set; 0: clipped away; -1: out of the fixed-point range
RENDER_HD inline int setup_line(const Camera& cam, const double* view, const float* a, const float* b, ScreenLine* out)
{
    double p[2][3];
    to_camera(view, a, p[0]);
    to_camera(view, b, p[1]);
    for (int k = 0; k < 6; k++) {
        const double d0 = plane_dist(cam, k, p[0][0], p[0][1], p[0][2]);
        const double d1 = plane_dist(cam, k, p[1][0], p[1][1], p[1][2]);
        const bool in0 = d0 >= 0.0, in1 = d1 >= 0.0;
        if (in0 && in1) continue;
        if (!in0 && !in1) return 0;
        const int i = in0 ? 0 : 1, o = 1 - i;               // from the inside end to the outside end
        const double di = in0 ? d0 : d1, dout = in0 ? d1 : d0;
        const double t = di / (di - dout);
        for (int j = 0; j < 3; j++) p[o][j] = p[i][j] + t * (p[o][j] - p[i][j]);
    }
    int32_t x[2], y[2];
    if (!project_pixel(cam, p[0], &x[0], &y[0]) || !project_pixel(cam, p[1], &x[1], &y[1])) return -1;
    const int s = (y[1] < y[0] || (y[1] == y[0] && x[1] < x[0])) ? 1 : 0;     // the start: lower in (y, x)
    out->x0 = x[s]; out->y0 = y[s]; out->x1 = x[1 - s]; out->y1 = y[1 - s];
    out->iz0 = 1.0 / p[s][2];
    out->iz1 = 1.0 / p[1 - s][2];
    const int32_t dx = out->x1 - out->x0, dy = out->y1 - out->y0;            // dy >= 0
    const int32_t adx = dx < 0 ? -dx : dx;
    out->sx = dx < 0 ? -1 : 1;
    out->xmajor = adx >= dy;
    out->n = out->xmajor ? adx : dy;
    out->dminor = out->xmajor ? dy : adx;
    int32_t lo, hi;
    if (out->xmajor) {
        lo = out->sx > 0 ? -out->x0 : out->x0 - (cam.w - 1);
        hi = out->sx > 0 ? cam.w - 1 - out->x0 : out->x0;
    } else {
        lo = -out->y0;
        hi = cam.h - 1 - out->y0;
    }
    out->k0 = lo > 0 ? lo : 0;
    out->k1 = hi < out->n ? hi : out->n;
    return 1;
}

// step k (0 .. n) of the walk: the pixel and its 1/Z
RENDER_HD inline void line_pixel(const ScreenLine& l, int32_t k, int32_t* x, int32_t* y, float* depth)
{
    const int64_t m = l.n > 0 ? (2 * (int64_t)k * l.dminor + l.n) / (2 * (int64_t)l.n) : 0;
    if (l.xmajor) {
        *x = l.x0 + l.sx * k;
        *y = l.y0 + (int32_t)m;
    } else {
        *x = l.x0 + l.sx * (int32_t)m;
        *y = l.y0 + k;
    }
    if (l.n > 0) *depth = (float)(((double)(l.n - k) * l.iz0 + (double)k * l.iz1) / (double)l.n);
    else *depth = (float)(l.iz0 > l.iz1 ? l.iz0 : l.iz1);
}

// a cloud point: true when it is inside the near / far range and the viewport
RENDER_HD inline bool setup_point(const Camera& cam, const double* view, const float* p, int32_t* px, int32_t* py,
                                  float* depth)
{
    double q[3];
    to_camera(view, p, q);
    if (!(q[2] >= cam.znear && q[2] <= cam.zfar)) return false;
    const double u = (cam.fx * q[0]) / q[2] + cam.cx, v = (cam.fy * q[1]) / q[2] + cam.cy;
    if (!(u >= 0.0 && u < (double)cam.w && v >= 0.0 && v < (double)cam.h)) return false;
    *px = (int32_t)u;
    *py = (int32_t)v;
    *depth = (float)(1.0 / q[2]);
    return true;
}

RENDER_HD inline uint32_t float_bits(float f)
{
    union { float f; uint32_t u; } v;
    v.f = f;
    return v.u;
}
RENDER_HD inline float bits_float(uint32_t u)
{
    union { float f; uint32_t u; } v;
    v.u = u;
    return v.f;
}

// the visibility key: a larger 1/Z (nearer) gives a smaller key; then the kind, then the index
RENDER_HD inline uint64_t depth_key(float depth, int kind, uint32_t index)
{
    return ((uint64_t)(~float_bits(depth)) << 32) | ((uint64_t)kind << kIndexBits) | (uint64_t)index;
}

}  // namespace render_setup

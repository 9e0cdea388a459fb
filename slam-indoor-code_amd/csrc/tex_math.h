// Per-face texture atlas: the arithmetic shared by the kernels (tex.hip) and the host
// twin (tex_host.cpp).  tests/tex_ref.py is the definition; every
// f64 expression below is written in the contract's order and is built without FMA
// contraction (-ffp-contract=off), every other step is integer, so host and device agree
// bit for bit.  Plain C++: it also compiles without HIP (tests/cpp/tex_host_test.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define TEX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TEX_HD inline
#endif

namespace slamhip {

constexpr int kTexMinT = 1, kTexMaxT = 64;         // texels per triangle leg
constexpr int kTexMargin = 4;                      // S = T + 4: the cell size
constexpr int kTexMaxPage = 8192;
constexpr int kTexMaxFaces = 1 << 30;
constexpr int kTexMaxMinPixels = 1 << 30;
constexpr int kTexMaxViews = 1 << 20;              // per fill call
constexpr int kTexFaceKind = 2;                    // the kind field of a rendered id (render.hip)

TEX_HD bool tex_finite(double v) { return v - v == 0.0; }

// The face index a rendered id counts for, or -1: kind 2 (face) and index < nf.  The
// background (-1) has kind 3.
TEX_HD int32_t tex_id_face(int32_t id, int nf)
{
    const uint32_t u = (uint32_t)id;
    if ((u >> 30) != (uint32_t)kTexFaceKind) return -1;
    const int32_t f = (int32_t)(u & 0x3fffffffu);
    return f < nf ? f : -1;
}

// one step of the selection rule: view m saw the face in c pixels
TEX_HD void tex_best_step(int32_t& best_count, int32_t& best_view, int32_t c, int32_t m)
{
    if (c > best_count || (c == best_count && c > 0 && m < best_view)) {
        best_count = c;
        best_view = m;
    }
}

// The layout, a pure function of (nf, T, page): cells of S x S texels in raster order,
// cells_x per row, cut into pages of cells_x rows.  All pages are page_w wide, so the
// atlas is one raster of cell rows: page p starts at texel row p * cells_x * S.
struct TexLayout {
    int T, S, cells_x, page_w;
    long long ncells, cell_rows;       // (nf + 1) / 2, ceil(ncells / cells_x)
    int npages;
};

TEX_HD bool tex_layout_args_ok(int T, int page) { return T >= kTexMinT && T <= kTexMaxT && page >= T + kTexMargin && page <= kTexMaxPage; }

TEX_HD TexLayout tex_layout(int nf, int T, int page)
{
    TexLayout l;
    l.T = T;
    l.S = T + kTexMargin;
    l.cells_x = page / l.S;
    l.page_w = l.cells_x * l.S;
    l.ncells = ((long long)nf + 1) >> 1;
    l.cell_rows = (l.ncells + l.cells_x - 1) / l.cells_x;
    l.npages = (int)((l.cell_rows + l.cells_x - 1) / l.cells_x);
    return l;
}

// texel rows of page p
TEX_HD int tex_page_height(const TexLayout& l, int p)
{
    const long long rows = l.cell_rows - (long long)p * l.cells_x;
    return l.S * (int)(rows < l.cells_x ? rows : l.cells_x);
}

// cell-local continuous coordinates of corner k (0 a, 1 b, 2 c) of a face in `half`
TEX_HD void tex_corner(int T, int half, int k, int& x, int& y)
{
    if (half == 0) {
        x = 1 + (k == 1 ? T : 0);
        y = 1 + (k == 2 ? T : 0);
    } else {
        x = T + 3 - (k == 1 ? T : 0);
        y = T + 3 - (k == 2 ? T : 0);
    }
}

// the half that owns texel (i, j) of a cell
TEX_HD int tex_half(int T, int i, int j) { return i + j <= T + 2 ? 0 : 1; }

// barycentric coordinates of the centre of texel (i, j), extrapolated from the half's mapping
TEX_HD void tex_bary(int T, int half, int i, int j, double& alpha, double& beta, double& gamma)
{
    const double xc = (double)i + 0.5, yc = (double)j + 0.5, t = (double)T;
    if (half == 0) {
        beta = (xc - 1.0) / t;
        gamma = (yc - 1.0) / t;
    } else {
        beta = ((double)(T + 3) - xc) / t;
        gamma = ((double)(T + 3) - yc) / t;
    }
    alpha = (1.0 - beta) - gamma;
}

TEX_HD double tex_mix(double alpha, double beta, double gamma, double a, double b, double c)
{
    return (alpha * a + beta * b) + gamma * c;
}

// the Gouraud fallback of one channel
TEX_HD uint8_t tex_fallback(double alpha, double beta, double gamma, uint8_t ca, uint8_t cb, uint8_t cc)
{
    double v = floor(tex_mix(alpha, beta, gamma, (double)ca, (double)cb, (double)cc) + 0.5);
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    return (uint8_t)v;
}

// One axis of the bilinear lookup: the clamped coordinate's two taps and its weight in 1/256.
// c is finite.
TEX_HD void tex_axis(double c, int n, int& i0, int& i1, int& wgt)
{
    const double hi = (double)(n - 1);
    c = c < 0.0 ? 0.0 : (c > hi ? hi : c);
    const double f = floor(c);
    i0 = (int)f;
    i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
    wgt = (int)floor((c - f) * 256.0 + 0.5);
}

// The frame's colour at the projection of (X, Y, Z), or false: behind the camera or a
// projection that is not finite (no NaN or infinity reaches an integer conversion).
// px: the frame, h x w x channels bytes; out: blue, green, red.
TEX_HD bool tex_sample(const double* P, double X, double Y, double Z, const uint8_t* px, int w, int h, int channels,
                       uint8_t* out)
{
    const double h0 = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
    const double h1 = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
    const double h2 = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
    if (!(h2 > 0.0)) return false;
    const double u = h0 / h2, v = h1 / h2;
    if (!tex_finite(u) || !tex_finite(v)) return false;
    int x0, x1, wx, y0, y1, wy;
    tex_axis(u, w, x0, x1, wx);
    tex_axis(v, h, y0, y1, wy);
    const uint8_t* r0 = px + (size_t)y0 * w * channels;
    const uint8_t* r1 = px + (size_t)y1 * w * channels;
    for (int c = 0; c < 3; c++) {
        const int k = channels == 3 ? c : 0;
        const int32_t top = (int32_t)r0[(size_t)x0 * channels + k] * (256 - wx) + (int32_t)r0[(size_t)x1 * channels + k] * wx;
        const int32_t bot = (int32_t)r1[(size_t)x0 * channels + k] * (256 - wx) + (int32_t)r1[(size_t)x1 * channels + k] * wx;
        out[c] = (uint8_t)((top * (256 - wy) + bot * wy + 32768) >> 16);
    }
    return true;
}

// what a fill needs of one view
struct TexView {
    double P[12];
    int32_t frame, pad;
};

// One atlas texel: column x of the atlas raster, texel row y counted over all pages.  The
// caller has checked the faces' indices (inside nv) and best_view (-1 .. nviews - 1).
TEX_HD void tex_texel(const TexLayout& l, int nf, int x, long long y, const double* V, const uint8_t* C, const int32_t* F,
                      const uint8_t* frames, int w, int h, int channels, const TexView* views, const int32_t* best_count,
                      const int32_t* best_view, int min_pixels, uint8_t* out)
{
    const int cx = x / l.S, i = x - cx * l.S;
    const long long row = y / l.S;
    const int j = (int)(y - row * l.S);
    const int half = tex_half(l.T, i, j);
    const long long f = 2 * (row * l.cells_x + cx) + half;
    if (f >= nf) {
        out[0] = out[1] = out[2] = 0;
        return;
    }
    double alpha, beta, gamma;
    tex_bary(l.T, half, i, j, alpha, beta, gamma);
    const int32_t a = F[3 * f], b = F[3 * f + 1], c = F[3 * f + 2];
    const int32_t bv = best_view[f];
    if (best_count[f] >= min_pixels && bv >= 0) {
        const double X = tex_mix(alpha, beta, gamma, V[3 * (size_t)a], V[3 * (size_t)b], V[3 * (size_t)c]);
        const double Y = tex_mix(alpha, beta, gamma, V[3 * (size_t)a + 1], V[3 * (size_t)b + 1], V[3 * (size_t)c + 1]);
        const double Z = tex_mix(alpha, beta, gamma, V[3 * (size_t)a + 2], V[3 * (size_t)b + 2], V[3 * (size_t)c + 2]);
        const TexView& vw = views[bv];
        if (tex_sample(vw.P, X, Y, Z, frames + (size_t)vw.frame * w * h * channels, w, h, channels, out)) return;
    }
    for (int k = 0; k < 3; k++)
        out[k] = tex_fallback(alpha, beta, gamma, C[3 * (size_t)a + k], C[3 * (size_t)b + k], C[3 * (size_t)c + k]);
}

}  // namespace slamhip

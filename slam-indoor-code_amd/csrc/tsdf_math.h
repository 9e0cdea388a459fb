// TSDF fusion and marching cubes: the arithmetic shared by the kernels (tsdf.hip) and
// the host twin (tsdf_host.cpp).  tests/tsdf_ref.py is the definition (DESIGN.md
// section 27); every f64 expression below is written in the contract's order and is
// built without FMA contraction (-ffp-contract=off), every integer step is exact, so
// host and device agree bit for bit.  Plain C++: it also compiles without HIP
// (tests/cpp/tsdf_host_test.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TSDF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TSDF_HD inline
#endif

namespace slamhip {

constexpr int kTsdfMinDim = 2, kTsdfMaxDim = 2048;
constexpr long long kTsdfMaxNodes = 1ll << 30;
constexpr int kTsdfMaxMaps = 1 << 20;          // per call, and per volume: 2^20 * 1024 stays inside int32
constexpr int kTsdfQ = 1024;
constexpr int kTsdfPlanes = 6;                 // D, W, CW, B, G, R

// a node's flag byte in the extraction scratch
constexpr uint8_t kTsdfMaskBits = 7;           // bit a: the node's +axis-a edge carries a vertex
constexpr int kTsdfFaceShift = 3;              // bits 3..5: the triangles of the node's cell (0..5)
constexpr uint8_t kTsdfKnown = 0x40, kTsdfInside = 0x80;

TSDF_HD bool tsdf_finite(double v) { return v - v == 0.0; }

// the six sums of one node
struct TsdfNode {
    int32_t D, W, CW, B, G, R;
};

// One map's contribution to the node at (X, Y, Z).  P: 3 x 4 row-major; inv: the map, W x H
// f32; px: the frame, W x H x channels bytes.  The order is the contract's: projection, the
// validity test (a NaN or an infinity fails a comparison and never reaches the integer
// conversion), the gather, r, the quantised distance, the colour near the surface.
TSDF_HD void tsdf_integrate_node(TsdfNode& n, const double* P, double X, double Y, double Z, const float* inv,
                                 const uint8_t* px, int W, int H, int channels, double trunc)
{
    const double h0 = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
    const double h1 = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
    const double h2 = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
    if (!(h2 > 0.0)) return;
    const double u = h0 / h2, v = h1 / h2;
    if (!(u >= -0.5 && u < (double)W - 0.5 && v >= -0.5 && v < (double)H - 0.5)) return;
    int ix = (int)floor(u + 0.5), iy = (int)floor(v + 0.5);
    ix = ix < W ? ix : W - 1;      // never taken (u + 0.5 < W is exact here); kept as a bound on the gather
    iy = iy < H ? iy : H - 1;
    const size_t o = (size_t)iy * W + ix;
    const float w = inv[o];
    if (!(w > 0.f)) return;
    double r = (1.0 / (double)w - h2) / trunc;
    if (!(r >= -1.0)) return;      // hidden behind the surface (r is never a NaN: trunc > 0, h2 > 0, 1 / w finite)
    if (r > 1.0) r = 1.0;
    n.D += (int32_t)floor(r * 1024.0 + 0.5);
    n.W += 1;
    if (r < 1.0) {
        const uint8_t* p = px + o * channels;
        n.CW += 1;
        n.B += p[0];
        n.G += channels == 3 ? p[1] : p[0];
        n.R += channels == 3 ? p[2] : p[0];
    }
}

TSDF_HD double tsdf_coord(double o, int i, double s) { return o + (double)i * s; }

// flags of one node: known iff W >= min_weight, inside iff known and D < 0
TSDF_HD uint8_t tsdf_node_flags(int32_t D, int32_t W, int min_weight)
{
    if (W < min_weight) return 0;
    return (uint8_t)(kTsdfKnown | (D < 0 ? kTsdfInside : 0));
}

// the owner corner of cube edge e = axis * 4 + rank: rank with a zero bit inserted at position axis
TSDF_HD int tsdf_edge_owner(int e)
{
    const int a = e >> 2, r = e & 3;
    return (r & ((1 << a) - 1)) | ((r >> a) << (a + 1));
}

TSDF_HD int tsdf_popc3(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1); }

// t = fa / (fa - fb) of an edge from owner a to far node b (exactly one of them inside)
TSDF_HD double tsdf_edge_t(int32_t Da, int32_t Wa, int32_t Db, int32_t Wb)
{
    const double fa = (double)Da / (double)Wa, fb = (double)Db / (double)Wb;
    return fa / (fa - fb);
}

// a node's colour channel: (2 sum + CW) / (2 CW) in integers, 0 without colour
TSDF_HD int32_t tsdf_node_color(int32_t sum, int32_t cw) { return cw ? (2 * sum + cw) / (2 * cw) : 0; }

TSDF_HD uint8_t tsdf_mix_color(int32_t ca, int32_t cb, double t)
{
    return (uint8_t)floor(((double)ca + t * ((double)cb - (double)ca)) + 0.5);
}

}  // namespace slamhip

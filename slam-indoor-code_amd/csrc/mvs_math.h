// Plane-sweep stereo: the arithmetic shared by the kernels (mvs.hip) and the host
// twin (mvs_host.cpp).  tests/mvs_ref.py is the definition;
// every f64 expression below is written in the contract's order and is built
// without FMA contraction (-ffp-contract=off), so host and device agree bit for bit.
// Plain C++: it also compiles without HIP (tests/cpp/mvs_host_test.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MVS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MVS_HD inline
#endif

namespace slamhip {

constexpr int kMvsMaxSources = 4, kMvsMinPlanes = 4, kMvsMaxPlanes = 256, kMvsMaxRadius = 3, kMvsMaxWidth = 4096;
constexpr int kMvsCensusRx = 4, kMvsCensusRy = 3;      // 9 x 7 window, 62 bits
constexpr int kMvsInvalidCost = 64;
constexpr int kMvsFilterBorder = 4;                    // the filter drops radius + 4 pixels at each side

// the fixed-point BGR -> gray of fast_detect
MVS_HD uint32_t mvs_gray(const uint8_t* p, int channels)
{
    if (channels == 1) return p[0];
    return ((uint32_t)p[0] * 1868u + (uint32_t)p[1] * 9617u + (uint32_t)p[2] * 4899u + (1u << 13)) >> 14;
}

MVS_HD int mvs_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

MVS_HD int mvs_popc64(uint64_t v)
{
    return __builtin_popcountll(v);
}

// q_i = (M[i][0] * x + M[i][1] * y) + M[i][2]: the part of the projection that no plane changes
MVS_HD void mvs_q(const double* M, int x, int y, double* q)
{
    const double fx = (double)x, fy = (double)y;
    q[0] = (M[0] * fx + M[1] * fy) + M[2];
    q[1] = (M[3] * fx + M[4] * fy) + M[5];
    q[2] = (M[6] * fx + M[7] * fy) + M[8];
}

// h = q + w v, (u, vv) = (h0, h1) / h2; valid iff h2 > 0 and the nearest pixel is inside W x H.
// A NaN or an infinity fails a comparison and never reaches the integer conversion.
MVS_HD bool mvs_project(const double* q, const double* v, double w, int W, int H, int* ix, int* iy, double* h2_out)
{
    const double h0 = q[0] + w * v[0];
    const double h1 = q[1] + w * v[1];
    const double h2 = q[2] + w * v[2];
    *h2_out = h2;
    if (!(h2 > 0.0)) return false;
    const double u = h0 / h2, vv = h1 / h2;
    if (!(u >= -0.5 && u < (double)W - 0.5 && vv >= -0.5 && vv < (double)H - 0.5)) return false;
    const int x = (int)floor(u + 0.5), y = (int)floor(vv + 0.5);
    *ix = x < W ? x : W - 1;     // never taken (u + 0.5 < W is exact here); kept as a bound on the gather
    *iy = y < H ? y : H - 1;
    return true;
}

// The winner rule as a stream over the planes d = 0 .. D - 1 of one pixel.  top holds
// the 4 smallest keys C << 8 | d (C <= 4 * 64 * 49 < 2^24, d < 256: the integer order
// is the lexicographic order of (C, d)), top[0] is the winner; a and c are C[best - 1]
// and C[best + 1], captured as the planes pass; nv is nvalid[best].
struct MvsPixel {
    uint32_t top[4];
    int32_t a, c, prev, nv;
};

MVS_HD void mvs_pixel_init(MvsPixel& p)
{
    p.top[0] = p.top[1] = p.top[2] = p.top[3] = 0xffffffffu;
    p.a = p.c = p.prev = p.nv = 0;
}

MVS_HD void mvs_pixel_update(MvsPixel& p, int d, int32_t C, int32_t nvalid)
{
    const uint32_t key = ((uint32_t)C << 8) | (uint32_t)d;
    if (d > 0 && (p.top[0] & 255u) == (uint32_t)(d - 1)) p.c = C;      // the plane after the winner so far
    if (key < p.top[0]) {                                              // strictly smaller C: d only grows
        p.a = p.prev;
        p.nv = nvalid;
    }
    // insertion into the sorted four
    uint32_t k = key;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t t = p.top[i];
        const bool lt = k < t;
        p.top[i] = lt ? k : t;
        k = lt ? t : k;
    }
    p.prev = C;
}

// plane, cost and the refined inverse depth (0 when the pixel is rejected)
MVS_HD void mvs_pixel_finish(const MvsPixel& p, const double* w, int D, int uniq, int min_views, int16_t* plane,
                             int32_t* cost, float* inv_depth)
{
    const int best = (int)(p.top[0] & 255u);
    const int32_t b = (int32_t)(p.top[0] >> 8);
    int32_t second = 0;
    bool have = false;
#pragma unroll
    for (int i = 1; i < 4; i++) {
        const int d = (int)(p.top[i] & 255u);
        const int gap = d > best ? d - best : best - d;
        if (!have && p.top[i] != 0xffffffffu && gap > 1) {
            second = (int32_t)(p.top[i] >> 8);
            have = true;
        }
    }
    *plane = (int16_t)best;
    *cost = b;
    const bool ok = have && (int64_t)b * 100 < (int64_t)uniq * second && p.nv >= min_views;
    float out = 0.f;
    if (ok) {
        double off = 0.0;
        if (best > 0 && best < D - 1) {
            const int32_t den = p.a - 2 * b + p.c;
            if (den > 0) off = (double)(p.a - p.c) / (double)(2 * den);
        }
        double wq = w[best];
        if (best > 0 && best < D - 1) {
            if (off >= 0.0)
                wq = w[best] + off * (w[best + 1] - w[best]);
            else
                wq = w[best] + off * (w[best] - w[best - 1]);
        }
        out = (float)wq;
    }
    *inv_depth = out;
}

// X = c + (B (x, y, 1)) * (1 / wi)
MVS_HD void mvs_backproject(const double* B, const double* c, int x, int y, float wi, double* X)
{
    const double fx = (double)x, fy = (double)y;
    const double s = 1.0 / (double)wi;
    X[0] = c[0] + ((B[0] * fx + B[1] * fy) + B[2]) * s;
    X[1] = c[1] + ((B[3] * fx + B[4] * fy) + B[5]) * s;
    X[2] = c[2] + ((B[6] * fx + B[7] * fy) + B[8]) * s;
}

// the pairwise consistency of a pixel of inverse depth wi against the neighbour's wj at its projection
MVS_HD bool mvs_consistent(double h2, float wj, float wi, double eps)
{
    return wj > 0.f && fabs(h2 * (double)wj / (double)wi - 1.0) <= eps;
}

MVS_HD bool mvs_finite(double v) { return v - v == 0.0; }

}  // namespace slamhip

// Semi-global aggregation of the plane-sweep cost volume: the arithmetic shared by
// the kernels (mvs_sgm.hip) and the host twin (mvs_sgm_host.cpp).
// tests/mvs_sgm_ref.py is the definition.  Integers only, so
// every schedule gives the same bits.  Plain C++: it also compiles without HIP
// (tests/cpp/mvs_sgm_host_test.cpp).
#pragma once

#include "mvs_math.h"

namespace slamhip {

constexpr int kSgmMaxCost = 64 * 49 * kMvsMaxSources;     // 12544: the largest C of the volume
constexpr int kSgmMaxP2 = 65535 - kSgmMaxCost;            // a path value C + P2 fits uint16
constexpr int kSgmMaxPenalty = 255;                       // p1, p2 per window pixel and source
constexpr uint32_t kSgmAbsent = 0x3fffffffu;              // a plane that does not exist: never the minimum, + P2 fits

// the paths in the contract's order; 4 paths are the first four
MVS_HD void sgm_dir(int r, int* dx, int* dy)
{
    const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1};
    const int DY[8] = {0, 0, 1, -1, 1, -1, -1, 1};
    *dx = DX[r];
    *dy = DY[r];
}

// scan lines of a direction: h rows, w columns or the w + h - 1 diagonals
MVS_HD int sgm_line_count(int dx, int dy, int w, int h)
{
    return dy == 0 ? h : (dx == 0 ? w : w + h - 1);
}

// line i of a direction: its first pixel (the one whose predecessor is outside) and its length
MVS_HD void sgm_line(int dx, int dy, int w, int h, int i, int* x0, int* y0, int* len)
{
    int x, y;                                  // the start for dx, dy >= 0, mirrored below
    if (dy == 0) {
        x = 0;
        y = i;
    } else if (dx == 0) {
        x = i;
        y = 0;
    } else if (i < h) {
        x = 0;
        y = i;
    } else {
        x = i - h + 1;
        y = 0;
    }
    const int nx = w - x, ny = h - y;          // pixels left along each axis
    *len = dy == 0 ? nx : (dx == 0 ? ny : (nx < ny ? nx : ny));
    *x0 = dx < 0 ? w - 1 - x : x;
    *y0 = dy < 0 ? h - 1 - y : y;
}

// L_r(p, d) from C(p, d), the predecessor's L_r at d, d - 1, d + 1 (kSgmAbsent where the plane
// does not exist) and its minimum m
MVS_HD uint32_t sgm_step(uint32_t c, uint32_t same, uint32_t below, uint32_t above, uint32_t m, uint32_t P1, uint32_t P2)
{
    uint32_t best = same;
    const uint32_t a = below + P1, b = above + P1, j = m + P2;
    best = a < best ? a : best;
    best = b < best ? b : best;
    best = j < best ? j : best;
    return c + best - m;
}

MVS_HD bool sgm_penalties_ok(int p1, int p2, int paths)
{
    return p1 >= 0 && p1 <= p2 && p2 <= kSgmMaxPenalty && (paths == 4 || paths == 8);
}

// the effective penalty of a reference with S sources at radius r
MVS_HD int sgm_effective(int p, int radius, int S) { return p * (2 * radius + 1) * (2 * radius + 1) * S; }

MVS_HD bool sgm_aggregate_args_ok(int n, int w, int h, int D, int P1, int P2, int paths)
{
    return n >= 0 && n <= 65535 && w >= 1 && h >= 1 && h <= (1 << 20) && D >= kMvsMinPlanes && D <= kMvsMaxPlanes &&
           P1 >= 0 && P1 <= P2 && P2 <= kSgmMaxP2 && (paths == 4 || paths == 8);
}

}  // namespace slamhip

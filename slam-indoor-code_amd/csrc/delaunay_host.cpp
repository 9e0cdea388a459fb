// slam_delaunay_2d_host: the contract of slam_delaunay_2d (delaunay.hip, DESIGN.md
// section 11) evaluated on the host, for components so small that a launch and
// its readbacks cost more than the whole triangulation (the scene driver sends
// components below 64 points here).  The same exact predicates (exact_pred.h),
// the same star walk from the nearest neighbour and the same cocircular tie
// rule, one vertex after the other; O(n^2) predicates, no device, no context.
#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/slamhip.h"
#include "exact_pred.h"

namespace {

struct P2 { float x, y; };

int orient(const P2& a, const P2& b, const P2& c) { return exact_pred::orient2d(a.x, a.y, b.x, b.y, c.x, c.y); }
int incircle(const P2& a, const P2& b, const P2& c, const P2& d)
{
    return exact_pred::incircle(a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y);
}

// apex of the directed edge (a, b) over the vertices V, or -1 (delaunay.hip, apex)
int apex(const P2* p, const std::vector<int>& V, int a, int b)
{
    int c = -1;
    bool tie = false;
    for (int v : V) {
        if (orient(p[a], p[b], p[v]) <= 0) continue;
        if (c < 0) { c = v; continue; }
        const int s = incircle(p[a], p[b], p[c], p[v]);
        if (s > 0) { c = v; tie = false; }
        else if (s == 0) tie = true;
    }
    if (c < 0 || !tie) return c;
    int tmin = INT_MAX, t1 = -1, t2 = -1;       // min index; first after b; last before a
    for (int v : V) {
        if (orient(p[a], p[b], p[v]) <= 0) continue;
        if (v != c && incircle(p[a], p[b], p[c], p[v]) != 0) continue;
        tmin = std::min(tmin, v);
        if (t1 < 0 || orient(p[b], p[t1], p[v]) < 0) t1 = v;
        if (t2 < 0 || orient(p[t2], p[a], p[v]) < 0) t2 = v;
    }
    if (tmin < a && tmin < b) return tmin;
    return a < b ? t1 : t2;
}

}  // namespace

extern "C" int slam_delaunay_2d_host(const float* xy, int n, int32_t* tris, int cap, int* n_tris)
{
    if (n < 0 || cap < 0 || !n_tris || (n > 0 && !xy) || (cap > 0 && !tris)) return SLAM_E_INVALID_ARG;
    *n_tris = 0;
    const P2* p = reinterpret_cast<const P2*>(xy);
    for (int i = 0; i < n; i++) {
        const bool ok = p[i].x >= -100000.f && p[i].x < 100000.f && p[i].y >= -100000.f && p[i].y < 100000.f;
        if (!ok) return SLAM_E_INVALID_ARG;        // Subdiv2D's rectangle; NaN fails every comparison
    }
    std::vector<int> V;
    for (int i = 0; i < n; i++) {
        bool dup = false;
        for (int j : V)
            if (p[j].x == p[i].x && p[j].y == p[i].y) { dup = true; break; }
        if (!dup) V.push_back(i);
    }
    std::vector<std::array<int32_t, 3>> out;
    const int nv = (int)V.size();
    for (int a : V) {
        int b0 = -1;
        for (int v : V)
            if (v != a && (b0 < 0 || exact_pred::closer(p[a].x, p[a].y, p[v].x, p[v].y, p[b0].x, p[b0].y) < 0)) b0 = v;
        if (b0 < 0) continue;
        int b = b0;
        bool closed = false;
        for (int step = 0; step < nv; step++) {          // counter-clockwise
            const int c = apex(p, V, a, b);
            if (c < 0) break;
            if (a < b && a < c) out.push_back({a, b, c});
            if (c == b0) { closed = true; break; }
            b = c;
        }
        if (closed) continue;
        b = b0;
        for (int step = 0; step < nv; step++) {          // clockwise from b0, up to the hull
            const int c = apex(p, V, b, a);
            if (c < 0) break;
            if (a < b && a < c) out.push_back({a, c, b});
            b = c;
        }
    }
    std::sort(out.begin(), out.end());
    *n_tris = (int)out.size();
    if ((int)out.size() > cap) return SLAM_E_CAPACITY;
    for (size_t t = 0; t < out.size(); t++)
        for (int q = 0; q < 3; q++) tris[3 * t + q] = out[t][q];
    return SLAM_OK;
}

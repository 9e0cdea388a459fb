// Chessboard labelling on the host: the board_w * board_h
// strongest corner candidates are accepted iff they form a complete lattice.
//
// Method: convex hull -> the four hull vertices spanning the largest
// quadrilateral are the board's outer corners -> the homography that takes them
// to the lattice's corners puts every point next to one lattice node; the
// labelling is accepted when each node receives exactly one point and the lattice
// is regular (the shared acceptance rule below).  Then the
// canonical one of the labelling's symmetries is taken: right-handed in image
// coordinates (y down), first corner with the least x + y (ties: least y).
// tests/calib_ref.py labels by peeling lines instead; the two must agree exactly.
// Everything is integer or f64 arithmetic on integer inputs in a fixed order:
// the result is deterministic.
#include "slamhip_internal.h"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace slamhip {

namespace {

struct Pt { long long x, y; };

long long cross(const Pt& o, const Pt& a, const Pt& b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }

// Andrew's monotone chain; collinear points are dropped
std::vector<int> hull(const std::vector<Pt>& p)
{
    std::vector<int> idx(p.size());
    std::iota(idx.begin(), idx.end(), 0);
    std::sort(idx.begin(), idx.end(), [&](int a, int b) { return p[a].x != p[b].x ? p[a].x < p[b].x : p[a].y < p[b].y; });
    std::vector<int> h;
    for (int pass = 0; pass < 2; pass++) {
        const size_t start = h.size();
        for (size_t k = 0; k < idx.size(); k++) {
            const int i = pass == 0 ? idx[k] : idx[idx.size() - 1 - k];
            while (h.size() >= start + 2 && cross(p[h[h.size() - 2]], p[h.back()], p[i]) <= 0) h.pop_back();
            h.push_back(i);
        }
        h.pop_back();
    }
    return h;
}

// H (row-major, h33 = 1) with H q[k] ~ d[k] for four correspondences; false: singular
bool homography4(const Pt* q, const double (*d)[2], double* H)
{
    double A[8][9];
    for (int k = 0; k < 4; k++) {
        const double x = (double)q[k].x, y = (double)q[k].y, u = d[k][0], v = d[k][1];
        const double r0[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, u};
        const double r1[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, v};
        std::copy(r0, r0 + 9, A[2 * k]);
        std::copy(r1, r1 + 9, A[2 * k + 1]);
    }
    for (int c = 0; c < 8; c++) {
        int piv = c;
        for (int r = c + 1; r < 8; r++)
            if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
        if (std::fabs(A[piv][c]) < 1e-12) return false;
        if (piv != c) std::swap_ranges(A[piv], A[piv] + 9, A[c]);
        for (int r = 0; r < 8; r++) {
            if (r == c) continue;
            const double f = A[r][c] / A[c][c];
            for (int k = c; k < 9; k++) A[r][k] -= f * A[c][k];
        }
    }
    for (int c = 0; c < 8; c++) H[c] = A[c][8] / A[c][c];
    H[8] = 1;
    return true;
}

// grid[i * bw + j]: the point at lattice node (column j, row i), by the homography of the quad
bool label_by_quad(const std::vector<Pt>& p, const int* quad, int bw, int bh, std::vector<int>& grid)
{
    const Pt q[4] = {p[quad[0]], p[quad[1]], p[quad[2]], p[quad[3]]};
    const double d[4][2] = {{0, 0}, {(double)bw - 1, 0}, {(double)bw - 1, (double)bh - 1}, {0, (double)bh - 1}};
    double H[9];
    if (!homography4(q, d, H)) return false;
    grid.assign((size_t)bw * bh, -1);
    for (size_t k = 0; k < p.size(); k++) {
        const double x = (double)p[k].x, y = (double)p[k].y;
        const double w = H[6] * x + H[7] * y + H[8];
        if (!(std::fabs(w) > 1e-12)) return false;
        const double u = (H[0] * x + H[1] * y + H[2]) / w, v = (H[3] * x + H[4] * y + H[5]) / w;
        const double ju = std::floor(u + 0.5), iv = std::floor(v + 0.5);
        // within 0.4 of a node: lens distortion bends the rows, clutter lands between them
        if (!(std::fabs(u - ju) < 0.4 && std::fabs(v - iv) < 0.4)) return false;
        if (ju < 0 || ju >= bw || iv < 0 || iv >= bh) return false;
        int& cell = grid[(size_t)iv * bw + (size_t)ju];
        if (cell >= 0) return false;
        cell = (int)k;
    }
    return true;   // bw * bh points, each in a cell of its own: every cell is taken
}

// The acceptance rule of a labelling (part of the contract, integer exact): along
// every row and column each inner node lies within a quarter of the local spacing
// of the midpoint of its two neighbours.
bool regular(const std::vector<Pt>& p, const std::vector<int>& grid, int bw, int bh)
{
    auto ok = [&](int a, int b, int c) {
        const Pt &A = p[grid[a]], &B = p[grid[b]], &C = p[grid[c]];
        const long long dx = 2 * B.x - A.x - C.x, dy = 2 * B.y - A.y - C.y;   // twice the deviation from the midpoint
        const long long sx = C.x - A.x, sy = C.y - A.y;                       // twice the spacing
        return 16 * (dx * dx + dy * dy) <= sx * sx + sy * sy;
    };
    for (int i = 0; i < bh; i++)
        for (int j = 1; j + 1 < bw; j++)
            if (!ok(i * bw + j - 1, i * bw + j, i * bw + j + 1)) return false;
    for (int j = 0; j < bw; j++)
        for (int i = 1; i + 1 < bh; i++)
            if (!ok((i - 1) * bw + j, i * bw + j, (i + 1) * bw + j)) return false;
    return true;
}

// ---- the lattice-growing labeller (tests/fisheye_ref.py
// label_board_grow is the definition, and this equals it index for index) ----

// the acceptance rule of a grown labelling: `regular`, and along every row and
// column the deviations from the midpoint change slowly (a lens bends a row, it
// does not kink it): 16 |2 dev_j - dev_(j-1) - dev_(j+1)|^2 <= |P_(j+2) - P_(j-2)|^2
bool smooth(const std::vector<Pt>& p, const std::vector<int>& grid, int bw, int bh)
{
    if (!regular(p, grid, bw, bh)) return false;
    // five consecutive nodes of a line, as grid positions
    auto ok = [&](int a0, int a1, int a2, int a3, int a4) {
        const Pt &A = p[grid[a0]], &B = p[grid[a1]], &C = p[grid[a2]], &D = p[grid[a3]], &E = p[grid[a4]];
        const long long d1x = 2 * B.x - A.x - C.x, d1y = 2 * B.y - A.y - C.y;
        const long long d2x = 2 * C.x - B.x - D.x, d2y = 2 * C.y - B.y - D.y;
        const long long d3x = 2 * D.x - C.x - E.x, d3y = 2 * D.y - C.y - E.y;
        const long long kx = 2 * d2x - d1x - d3x, ky = 2 * d2y - d1y - d3y;
        const long long sx = E.x - A.x, sy = E.y - A.y;
        return 16 * (kx * kx + ky * ky) <= sx * sx + sy * sy;
    };
    for (int i = 0; i < bh; i++)
        for (int j = 2; j + 2 < bw; j++)
            if (!ok(i * bw + j - 2, i * bw + j - 1, i * bw + j, i * bw + j + 1, i * bw + j + 2)) return false;
    for (int j = 0; j < bw; j++)
        for (int i = 2; i + 2 < bh; i++)
            if (!ok((i - 2) * bw + j, (i - 1) * bw + j, i * bw + j, (i + 1) * bw + j, (i + 2) * bw + j)) return false;
    return true;
}

constexpr int kGrowFactor = 2;   // the 2 * bw * bh strongest candidates are the input
constexpr int kGrowSeeds = 8;    // seeds are tried until a board is found and this seed index is reached
// ... and never more than bw * bh + kGrowSeeds + 1 of them: at most bw * bh of the candidates are
// no corner of a complete board, so that many seeds hold at least kGrowSeeds + 1 of its corners

// grid (bh x bw, indices into p) of the best complete window over all seeds; false: none
bool grow_lattice(const std::vector<Pt>& p, const std::vector<long long>& resp, int bw, int bh, std::vector<int>& out)
{
    const int m = (int)p.size(), n = bw * bh, lim = std::max(bw, bh), side = 2 * lim + 1;
    auto d2 = [&](const Pt& a, const Pt& b) { return (a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y); };
    // the index of the point nearest to q, ties to the lower index
    auto nearest = [&](const Pt& q, long long& dist) {
        int k = 0;
        dist = d2(p[0], q);
        for (int i = 1; i < m; i++) {
            const long long d = d2(p[i], q);
            if (d < dist) { dist = d; k = i; }
        }
        return k;
    };
    struct Node { int pt; Pt u, v; };
    bool have = false;
    long long best = 0;
    std::vector<Node> lab((size_t)side * side);
    std::vector<char> used(m);
    std::vector<int> grid(n), nb;
    const int seeds = std::min(m, n + kGrowSeeds + 1);
    for (int s = 0; s < seeds; s++) {
        // the seed's four nearest neighbours, ties to the lower index
        nb.clear();
        for (int i = 0; i < m; i++)
            if (i != s) nb.push_back(i);
        const int cnt = std::min(4, (int)nb.size());
        std::partial_sort(nb.begin(), nb.begin() + cnt, nb.end(), [&](int a, int b) {
            const long long da = d2(p[a], p[s]), db = d2(p[b], p[s]);
            return da != db ? da < db : a < b;
        });
        bool basis = false;
        Pt u{0, 0}, v{0, 0};
        if (cnt >= 1) {
            u = Pt{p[nb[0]].x - p[s].x, p[nb[0]].y - p[s].y};
            const long long uu = u.x * u.x + u.y * u.y;
            // the nearest roughly perpendicular one (|cos| < 0.5) shorter than 2 |u|
            for (int k = 1; k < cnt && !basis; k++) {
                const Pt w{p[nb[k]].x - p[s].x, p[nb[k]].y - p[s].y};
                const long long ww = w.x * w.x + w.y * w.y, uw = u.x * w.x + u.y * w.y;
                if (4 * uw * uw < uu * ww && ww < 4 * uu) { v = w; basis = true; }
            }
        }
        if (basis) {
            for (auto& nd : lab) nd.pt = -1;
            std::fill(used.begin(), used.end(), 0);
            auto at = [&](int i, int j) -> Node& { return lab[(size_t)(i + lim) * side + (j + lim)]; };
            at(0, 0) = Node{s, u, v};
            used[s] = 1;
            int count = 1;
            std::vector<std::pair<int, int>> front{{0, 0}}, next;
            static const int dirs[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};
            while (!front.empty()) {
                next.clear();
                for (const auto& f : front) {
                    const int i = f.first, j = f.second;
                    const Node cur = at(i, j);
                    const Pt c = p[cur.pt];
                    for (const auto& dir : dirs) {
                        const int di = dir[0], dj = dir[1], qi = i + di, qj = j + dj;
                        if (qi < -lim || qi > lim || qj < -lim || qj > lim || at(qi, qj).pt >= 0) continue;
                        const Pt step{cur.u.x * di + cur.v.x * dj, cur.u.y * di + cur.v.y * dj};
                        const int bi = i - di, bj = j - dj;
                        const bool back = bi >= -lim && bi <= lim && bj >= -lim && bj <= lim && at(bi, bj).pt >= 0;
                        // twice the node minus the one behind it, else one local step ahead
                        const Pt pred = back ? Pt{2 * c.x - p[at(bi, bj).pt].x, 2 * c.y - p[at(bi, bj).pt].y}
                                             : Pt{c.x + step.x, c.y + step.y};
                        long long e;
                        const int k = nearest(pred, e);
                        // within 0.3 of the local step, and not taken
                        if (100 * e > 9 * (step.x * step.x + step.y * step.y) || used[k]) continue;
                        const Pt ns{p[k].x - c.x, p[k].y - c.y};
                        at(qi, qj) = di ? Node{k, Pt{ns.x * di, ns.y * di}, cur.v} : Node{k, cur.u, Pt{ns.x * dj, ns.y * dj}};
                        used[k] = 1;
                        count++;
                        next.emplace_back(qi, qj);
                    }
                }
                front.swap(next);
            }
            if (count >= n) {
                int i0 = lim, i1 = -lim, j0 = lim, j1 = -lim;
                for (int i = -lim; i <= lim; i++)
                    for (int j = -lim; j <= lim; j++)
                        if (at(i, j).pt >= 0) {
                            i0 = std::min(i0, i); i1 = std::max(i1, i);
                            j0 = std::min(j0, j); j1 = std::max(j1, j);
                        }
                // the complete windows, as labelled and (oblong boards) turned by a quarter
                for (int o = 0; o < (bw == bh ? 1 : 2); o++) {
                    const int W = o == 0 ? bw : bh, H = o == 0 ? bh : bw;
                    for (int oi = i0; oi <= i1 - W + 1; oi++)
                        for (int oj = j0; oj <= j1 - H + 1; oj++) {
                            bool complete = true;
                            for (int a = 0; a < W && complete; a++)
                                for (int b = 0; b < H && complete; b++) complete = at(oi + a, oj + b).pt >= 0;
                            if (!complete) continue;
                            for (int a = 0; a < W; a++)
                                for (int b = 0; b < H; b++) {
                                    const int node = at(oi + a, oj + b).pt;
                                    if (o == 0) grid[(size_t)b * bw + a] = node;
                                    else grid[(size_t)a * bw + b] = node;
                                }
                            if (!smooth(p, grid, bw, bh)) continue;
                            long long score = 0;
                            for (int k = 0; k < n; k++) score += resp[grid[k]];
                            if (!have || score > best) { have = true; best = score; out = grid; }
                        }
                }
            }
        }
        if (have && s >= kGrowSeeds) break;
    }
    return have;
}

// the canonical one of a labelling's symmetries, written as corners: right-handed
// ones only, then the least first corner; false: none is right-handed
bool write_canonical(const std::vector<Pt>& p, const std::vector<int>& grid, int scale, int bw, int bh, float* corners)
{
    auto at = [&](int i, int j) -> const Pt& { return p[grid[(size_t)i * bw + j]]; };
    const bool flip = cross(at(0, 0), at(0, 1), at(1, 0)) < 0;
    auto node = [&](int rot, int i, int j) -> const Pt& {
        // rot 0: as labelled; 1: by 180 degrees; 2, 3: by a quarter turn either way (square boards)
        int si = i, sj = j;
        if (rot == 1) { si = bh - 1 - i; sj = bw - 1 - j; }
        else if (rot == 2) { si = j; sj = bw - 1 - i; }
        else if (rot == 3) { si = bh - 1 - j; sj = i; }
        return at(si, flip ? bw - 1 - sj : sj);
    };
    const int nrot = bw == bh ? 4 : 2;
    int pick = -1;
    for (int r = 0; r < nrot; r++) {
        if (cross(node(r, 0, 0), node(r, 0, 1), node(r, 1, 0)) <= 0) continue;
        if (pick < 0) { pick = r; continue; }
        const Pt &a = node(r, 0, 0), &b = node(pick, 0, 0);
        if (a.x + a.y < b.x + b.y || (a.x + a.y == b.x + b.y && a.y < b.y)) pick = r;
    }
    if (pick < 0) return false;
    const float fs = (float)scale, off = (float)((scale - 1) / 2.0);
    for (int i = 0; i < bh; i++)
        for (int j = 0; j < bw; j++) {
            const Pt& z = node(pick, i, j);
            corners[2 * ((size_t)i * bw + j)] = fs * (float)z.x + off;
            corners[2 * ((size_t)i * bw + j) + 1] = fs * (float)z.y + off;
        }
    return true;
}

}  // namespace

bool label_chessboard_grow(const int32_t* cand, int n, int scale, int bw, int bh, float* corners)
{
    const int need = bw * bh;
    if (bw < 2 || bh < 2 || n < need) return false;
    // the strongest kGrowFactor * need, ties to the lower raster index (the input order)
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cand[3 * a + 2] > cand[3 * b + 2]; });
    const int m = std::min(n, kGrowFactor * need);
    std::vector<Pt> p(m);
    std::vector<long long> resp(m);
    for (int k = 0; k < m; k++) {
        p[k] = Pt{cand[3 * order[k]], cand[3 * order[k] + 1]};
        resp[k] = cand[3 * order[k] + 2];
    }
    for (int a = 0; a < m; a++)
        for (int b = a + 1; b < m; b++)
            if (p[a].x == p[b].x && p[a].y == p[b].y) return false;
    std::vector<int> grid;
    return grow_lattice(p, resp, bw, bh, grid) && write_canonical(p, grid, scale, bw, bh, corners);
}

bool label_chessboard(const int32_t* cand, int n, int scale, int bw, int bh, float* corners)
{
    const int need = bw * bh;
    if (bw < 2 || bh < 2 || n < need) return false;
    // the strongest `need`, ties to the lower raster index (the input order)
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cand[3 * a + 2] > cand[3 * b + 2]; });
    std::vector<Pt> p(need);
    for (int k = 0; k < need; k++) p[k] = Pt{cand[3 * order[k]], cand[3 * order[k] + 1]};
    for (int a = 0; a < need; a++)
        for (int b = a + 1; b < need; b++)
            if (p[a].x == p[b].x && p[a].y == p[b].y) return false;

    const std::vector<int> h = hull(p);
    const int nh = (int)h.size();
    if (nh < 4) return false;
    long long best = -1;
    int quad[4] = {0, 0, 0, 0};
    for (int a = 0; a < nh; a++)
        for (int b = a + 1; b < nh; b++)
            for (int c = b + 1; c < nh; c++)
                for (int d = c + 1; d < nh; d++) {
                    const long long s = cross(p[h[a]], p[h[b]], p[h[c]]) + cross(p[h[a]], p[h[c]], p[h[d]]);
                    const long long area = s < 0 ? -s : s;
                    if (area > best) {
                        best = area;
                        quad[0] = h[a]; quad[1] = h[b]; quad[2] = h[c]; quad[3] = h[d];
                    }
                }
    std::vector<int> grid;
    bool ok = label_by_quad(p, quad, bw, bh, grid) && regular(p, grid, bw, bh);
    if (!ok) {
        // the other pairing of hull edges with the board's sides
        const int q2[4] = {quad[1], quad[2], quad[3], quad[0]};
        ok = label_by_quad(p, q2, bw, bh, grid) && regular(p, grid, bw, bh);
    }
    if (!ok) return false;

    return write_canonical(p, grid, scale, bw, bh, corners);
}

}  // namespace slamhip

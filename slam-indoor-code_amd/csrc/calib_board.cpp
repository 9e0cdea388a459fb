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

}  // namespace

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

    // the symmetries: index maps (i, j) -> node; right-handed ones only, then the least first corner
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

}  // namespace slamhip

// Exact geometric predicates on f32 coordinates for the Delaunay step
// (delaunay.hip), host and device, header only.  Each returns the exact sign
// in {-1, 0, +1} of
//
//   orient2d(a, b, c)     | ax - cx   ay - cy |        > 0: c strictly left of a -> b
//                         | bx - cx   by - cy |
//   incircle(a, b, c, d)  the 3 x 3 lifted determinant of a - d, b - d, c - d
//                         > 0: d strictly inside the circle of the counter-clockwise a, b, c
//   closer(a, p, q)       |p - a|^2 - |q - a|^2        < 0: p strictly nearer to a than q
//
// as a filtered f64 evaluation followed, when the filter cannot decide, by an
// exact one.  *_filter returns kPredUndecided (2) instead of falling through
// (tests/cpp/exact_pred_test.cpp checks that it never returns a wrong sign).
//
// Filters.  The differences are taken in f64 and may round (1e-30 next to 9e4
// does).  orient2d and incircle are Shewchuk's stage A ("Adaptive Precision
// Floating-Point Arithmetic and Fast Robust Geometric Predicates", 1997,
// section 4): |det - exact| <= (3 + 16 e) e * (|l| + |r|), resp.
// (10 + 96 e) e * permanent, e = 2^-53, which hold for rounded differences as
// long as nothing over- or underflows.  closer: each squared difference carries
// three roundings, each sum one more and the final subtraction one, so
// |r - exact| <= ((1 + e)^4 - 1 + e (1 + e)^4) (d1 + d2) <= (5 e + 12 e^2) (d1 + d2),
// and the computed d1 + d2 is at least (1 - 6 e) times the exact one; 8 e times
// the computed sum covers it, and 8 e = 2^-50 scales exactly.
//
// Exact path.  No differences: the determinant is expanded in the raw
// coordinates.  A product of two f32 is exact in f64 (48 <= 53 bits); a product
// of four is the exact pair (hi, lo) of an FMA two-product of two such doubles.
// The terms (6 for orient2d, 8 for closer, 96 for incircle) are added into a
// non-overlapping expansion with two-sums (Shewchuk's grow-expansion with zero
// elimination); the sign of the exact sum is the sign of its largest component.
//
// Range.  Callers pass finite coordinates of magnitude at most 2^17 (delaunay.hip
// rejects anything outside [-100000, 100000) first).  A non-zero f32 is at least
// 2^-149 in magnitude, so a product of four is at least 2^-596 and its low part
// at least 2^-702: nothing underflows in f64 (2^-1074), and 96 terms below
// 2^69 overflow nothing.
//
// Build with -ffp-contract=off: the only fused operation is the explicit fma of
// two_prod.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EXACT_PRED_HD __host__ __device__
#else
#define EXACT_PRED_HD
#endif

namespace exact_pred {

constexpr int kPredUndecided = 2;
constexpr double kEps = 1.1102230246251565e-16;                  // 2^-53
constexpr double kOrientBound = (3.0 + 16.0 * kEps) * kEps;      // Shewchuk's ccwerrboundA
constexpr double kIncircleBound = (10.0 + 96.0 * kEps) * kEps;   // Shewchuk's iccerrboundA
constexpr double kCloserBound = 8.0 * kEps;                      // 2^-50

EXACT_PRED_HD inline int sign_of(double v) { return (v > 0.0) - (v < 0.0); }

// ---- filters ---------------------------------------------------------------------

EXACT_PRED_HD inline int orient2d_filter(float ax, float ay, float bx, float by, float cx, float cy)
{
    const double l = ((double)ax - (double)cx) * ((double)by - (double)cy);
    const double r = ((double)ay - (double)cy) * ((double)bx - (double)cx);
    const double det = l - r;
    double sum;
    if (l > 0.0) {
        if (r <= 0.0) return sign_of(det);
        sum = l + r;
    } else if (l < 0.0) {
        if (r >= 0.0) return sign_of(det);
        sum = -l - r;
    } else {
        return sign_of(det);
    }
    const double bound = kOrientBound * sum;
    if (det >= bound || -det >= bound) return sign_of(det);
    return kPredUndecided;
}

EXACT_PRED_HD inline int incircle_filter(float ax, float ay, float bx, float by, float cx, float cy, float dx, float dy)
{
    const double adx = (double)ax - (double)dx, ady = (double)ay - (double)dy;
    const double bdx = (double)bx - (double)dx, bdy = (double)by - (double)dy;
    const double cdx = (double)cx - (double)dx, cdy = (double)cy - (double)dy;
    const double bdxcdy = bdx * cdy, cdxbdy = cdx * bdy;
    const double alift = adx * adx + ady * ady;
    const double cdxady = cdx * ady, adxcdy = adx * cdy;
    const double blift = bdx * bdx + bdy * bdy;
    const double adxbdy = adx * bdy, bdxady = bdx * ady;
    const double clift = cdx * cdx + cdy * cdy;
    const double det = alift * (bdxcdy - cdxbdy) + blift * (cdxady - adxcdy) + clift * (adxbdy - bdxady);
    const double permanent = (fabs(bdxcdy) + fabs(cdxbdy)) * alift + (fabs(cdxady) + fabs(adxcdy)) * blift +
                             (fabs(adxbdy) + fabs(bdxady)) * clift;
    const double bound = kIncircleBound * permanent;
    if (det > bound || -det > bound) return sign_of(det);
    return kPredUndecided;
}

EXACT_PRED_HD inline int closer_filter(float ax, float ay, float px, float py, float qx, float qy)
{
    const double pdx = (double)px - (double)ax, pdy = (double)py - (double)ay;
    const double qdx = (double)qx - (double)ax, qdy = (double)qy - (double)ay;
    const double d1 = pdx * pdx + pdy * pdy, d2 = qdx * qdx + qdy * qdy;
    const double r = d1 - d2;
    const double bound = kCloserBound * (d1 + d2);
    if (r > bound || -r > bound) return sign_of(r);
    return kPredUndecided;
}

// ---- exact sums --------------------------------------------------------------------

// x + y = a + b exactly (Knuth)
EXACT_PRED_HD inline void two_sum(double a, double b, double& x, double& y)
{
    x = a + b;
    const double bv = x - a, av = x - bv;
    y = (a - av) + (b - bv);
}

// x + y = a * b exactly
EXACT_PRED_HD inline void two_prod(double a, double b, double& x, double& y)
{
    x = a * b;
    y = fma(a, b, -x);
}

// e[0 .. m): a non-overlapping expansion, components of increasing magnitude,
// no zeros.  Adds b in place; returns the new length (at most m + 1).
EXACT_PRED_HD inline int grow_expansion(double* e, int m, double b)
{
    double q = b;
    int h = 0;
    for (int i = 0; i < m; i++) {
        double s, lo;
        two_sum(q, e[i], s, lo);
        q = s;
        if (lo != 0.0) e[h++] = lo;        // h <= i: the slot has been read already
    }
    if (q != 0.0) e[h++] = q;
    return h;
}

EXACT_PRED_HD inline int expansion_sign(const double* e, int m) { return m ? sign_of(e[m - 1]) : 0; }

EXACT_PRED_HD inline int orient2d_exact(float ax, float ay, float bx, float by, float cx, float cy)
{
    // (ax - cx)(by - cy) - (ay - cy)(bx - cx); the two cx * cy cancel
    const double x0 = ax, y0 = ay, x1 = bx, y1 = by, x2 = cx, y2 = cy;
    const double t[6] = {x0 * y1, -(x0 * y2), -(x2 * y1), -(y0 * x1), y0 * x2, y2 * x1};
    double e[6];
    int m = 0;
    for (int i = 0; i < 6; i++) m = grow_expansion(e, m, t[i]);
    return expansion_sign(e, m);
}

EXACT_PRED_HD inline int closer_exact(float ax, float ay, float px, float py, float qx, float qy)
{
    const double a0 = ax, a1 = ay, p0 = px, p1 = py, q0 = qx, q1 = qy;
    const double t[8] = {p0 * p0, -2.0 * (p0 * a0), p1 * p1, -2.0 * (p1 * a1),
                         -(q0 * q0), 2.0 * (q0 * a0), -(q1 * q1), 2.0 * (q1 * a1)};
    double e[8];
    int m = 0;
    for (int i = 0; i < 8; i++) m = grow_expansion(e, m, t[i]);
    return expansion_sign(e, m);
}

// The lifted 4 x 4 determinant | x y x^2+y^2 1 | over the rows a, b, c, d equals
// the 3 x 3 one of the differences (subtract row d, then add 2 dx, 2 dy times
// the first two columns to the third).  Expanded along the column of ones:
//   + M(a, b, c) - M(a, b, d) + M(a, c, d) - M(b, c, d),
//   M(p, q, r) = sum over the permutations (P, Q, R) of (p, q, r) of
//                sgn * x_P * y_Q * (x_R^2 + y_R^2).
EXACT_PRED_HD inline int incircle_exact(float ax, float ay, float bx, float by, float cx, float cy, float dx, float dy)
{
    const double x[4] = {ax, bx, cx, dx}, y[4] = {ay, by, cy, dy};
    double w0[4], w1[4];
    for (int i = 0; i < 4; i++) { w0[i] = x[i] * x[i]; w1[i] = y[i] * y[i]; }
    double e[96];
    int m = 0;
    for (int skip = 3; skip >= 0; skip--) {
        int r[3], k = 0;
        for (int i = 0; i < 4; i++)
            if (i != skip) r[k++] = i;
        const double ms = ((3 - skip) & 1) ? -1.0 : 1.0;      // skip d: +, c: -, b: +, a: -
        for (int p = 0; p < 3; p++) {
            const int P = r[p], Q1 = r[(p + 1) % 3], R1 = r[(p + 2) % 3];
            // even permutation (P, Q1, R1) and the odd one (P, R1, Q1)
            const double xy_even = ms * (x[P] * y[Q1]), xy_odd = -ms * (x[P] * y[R1]);
            double hi, lo;
            two_prod(xy_even, w0[R1], hi, lo); m = grow_expansion(e, m, lo); m = grow_expansion(e, m, hi);
            two_prod(xy_even, w1[R1], hi, lo); m = grow_expansion(e, m, lo); m = grow_expansion(e, m, hi);
            two_prod(xy_odd, w0[Q1], hi, lo);  m = grow_expansion(e, m, lo); m = grow_expansion(e, m, hi);
            two_prod(xy_odd, w1[Q1], hi, lo);  m = grow_expansion(e, m, lo); m = grow_expansion(e, m, hi);
        }
    }
    return expansion_sign(e, m);
}

// ---- the predicates ------------------------------------------------------------------

EXACT_PRED_HD inline int orient2d(float ax, float ay, float bx, float by, float cx, float cy)
{
    const int s = orient2d_filter(ax, ay, bx, by, cx, cy);
    return s != kPredUndecided ? s : orient2d_exact(ax, ay, bx, by, cx, cy);
}

EXACT_PRED_HD inline int incircle(float ax, float ay, float bx, float by, float cx, float cy, float dx, float dy)
{
    const int s = incircle_filter(ax, ay, bx, by, cx, cy, dx, dy);
    return s != kPredUndecided ? s : incircle_exact(ax, ay, bx, by, cx, cy, dx, dy);
}

EXACT_PRED_HD inline int closer(float ax, float ay, float px, float py, float qx, float qy)
{
    const int s = closer_filter(ax, ay, px, py, qx, qy);
    return s != kPredUndecided ? s : closer_exact(ax, ay, px, py, qx, qy);
}

}  // namespace exact_pred

// calibrateCamera on the host, f64: the optimum of
//   sum over views and points of | project(K, D, R_v, t_v, X) - x |^2
// over fx fy cx cy, k1 k2 p1 p2 k3 and six extrinsic parameters per view, the
// model and free parameters of cv::calibrateCamera with default flags.  The
// contract is the optimum, not OpenCV's iterate after 30 steps.
//
// Initial values as OpenCV's: principal point at the image centre, fx fy from
// the vanishing-point equations of the per-view homographies (normalised DLT),
// poses from K^-1 H orthonormalised, distortion 0.  Then Levenberg-Marquardt on
// the normal equations with analytic Jacobians until the cost stops moving.
//
// Rotations are held as matrices and stepped on the left, R <- exp(d) R, so the
// Jacobian of a view's rotation is d(R X)/d d = -[R X]x at d = 0: no derivative
// of Rodrigues' formula is needed.  exp(d) and the final rotation vectors come
// from slam_rodrigues (pnp.hip); there is no second Rodrigues here.
//
// fisheye_calibrate is the same optimisation for the
// model of cv::fisheye::calibrate with the skew fixed at 0: fx fy cx cy, k1 k2
// k3 k4 and the poses, through the same Levenberg-Marquardt loop.  Its initial
// values are OpenCV's: f = max(w, h) / pi, the principal point at the centre,
// poses from the homographies of the points undistorted with D = 0.
#include "slamhip_internal.h"

#include "fisheye_math.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

namespace slamhip {

namespace {

constexpr int kIntr = 9;          // fx fy cx cy k1 k2 p1 p2 k3
constexpr int kIntrFisheye = 8;   // fx fy cx cy k1 k2 k3 k4

// in-place Gaussian elimination with partial pivoting of the n x n system A x = b; false: singular
bool solve_dense(std::vector<double>& A, std::vector<double>& b, int n)
{
    for (int c = 0; c < n; c++) {
        int piv = c;
        for (int r = c + 1; r < n; r++)
            if (std::fabs(A[(size_t)r * n + c]) > std::fabs(A[(size_t)piv * n + c])) piv = r;
        const double d = A[(size_t)piv * n + c];
        if (!(std::fabs(d) > 0) || !std::isfinite(d)) return false;
        if (piv != c) {
            for (int k = 0; k < n; k++) std::swap(A[(size_t)piv * n + k], A[(size_t)c * n + k]);
            std::swap(b[piv], b[c]);
        }
        for (int r = c + 1; r < n; r++) {
            const double f = A[(size_t)r * n + c] / d;
            if (f == 0) continue;
            for (int k = c; k < n; k++) A[(size_t)r * n + k] -= f * A[(size_t)c * n + k];
            b[r] -= f * b[c];
        }
    }
    for (int r = n - 1; r >= 0; r--) {
        double s = b[r];
        for (int k = r + 1; k < n; k++) s -= A[(size_t)r * n + k] * b[k];
        b[r] = s / A[(size_t)r * n + r];
    }
    return true;
}

// Hartley's normalisation of n 2-D points: T = [s 0 -s mx; 0 s -s my; 0 0 1]; false: all points equal
bool normalise(const double* p, int n, double* T)
{
    double mx = 0, my = 0;
    for (int i = 0; i < n; i++) { mx += p[2 * i]; my += p[2 * i + 1]; }
    mx /= n; my /= n;
    double d = 0;
    for (int i = 0; i < n; i++) d += std::hypot(p[2 * i] - mx, p[2 * i + 1] - my);
    d /= n;
    if (!(d > 1e-12) || !std::isfinite(d)) return false;
    const double s = std::sqrt(2.0) / d;
    const double t[9] = {s, 0, -s * mx, 0, s, -s * my, 0, 0, 1};
    std::memcpy(T, t, sizeof(t));
    return true;
}

void mul33(const double* a, const double* b, double* c)
{
    double r[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
    std::memcpy(c, r, sizeof(r));
}

// the homography board plane -> image by the normalised DLT (least squares with h33 = 1
// in normalised coordinates, where the board's centroid maps to the image points' centroid)
bool homography(const double* xy, const double* uv, int n, double* H)
{
    double Ta[9], Tb[9];
    if (!normalise(xy, n, Ta) || !normalise(uv, n, Tb)) return false;
    std::vector<double> N(64, 0.0), rhs(8, 0.0);
    for (int i = 0; i < n; i++) {
        const double x = Ta[0] * xy[2 * i] + Ta[2], y = Ta[4] * xy[2 * i + 1] + Ta[5];
        const double u = Tb[0] * uv[2 * i] + Tb[2], v = Tb[4] * uv[2 * i + 1] + Tb[5];
        const double r0[8] = {x, y, 1, 0, 0, 0, -u * x, -u * y};
        const double r1[8] = {0, 0, 0, x, y, 1, -v * x, -v * y};
        for (int a = 0; a < 8; a++) {
            for (int b = 0; b < 8; b++) N[a * 8 + b] += r0[a] * r0[b] + r1[a] * r1[b];
            rhs[a] += r0[a] * u + r1[a] * v;
        }
    }
    double scale = 0;
    for (int a = 0; a < 8; a++) scale = std::max(scale, std::fabs(N[a * 8 + a]));
    std::vector<double> M = N, x = rhs;
    if (!solve_dense(M, x, 8)) return false;
    // a rank-deficient system (collinear points) leaves a pivot at rounding level
    for (int a = 0; a < 8; a++)
        if (!(std::fabs(M[a * 8 + a]) > 1e-11 * scale)) return false;
    const double h[9] = {x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], 1};
    // H = Tb^-1 h Ta
    const double is = 1.0 / Tb[0];
    const double Tbi[9] = {is, 0, -Tb[2] * is, 0, is, -Tb[5] * is, 0, 0, 1};
    mul33(h, Ta, H);
    mul33(Tbi, H, H);
    if (!(std::fabs(H[8]) > 1e-300)) return false;
    for (int k = 0; k < 9; k++) H[k] /= H[8];
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(H[k])) return false;
    return true;
}

struct Problem {
    int nviews, npts;
    const float* obj;      // npts x 3, z = 0
    const float* img;      // nviews x npts x 2
    int nintr;             // kIntr, or kIntrFisheye for the fisheye model
};

// view_terms for the fisheye model: u = fx a g(r) + cx, v = fy b g(r) + cy with (a, b) = (Yx, Yy) / Yz,
// r = |(a, b)|, theta = atan r, g = theta_d / r (1 at r = 0); Ji is 2 x 8 per point
void fisheye_terms(const Problem& P, int v, const double* in, const double* R, const double* t, double* res, double* Ji,
                   double* Je)
{
    const double fx = in[0], fy = in[1], cx = in[2], cy = in[3];
    const double* k = in + 4;
    for (int i = 0; i < P.npts; i++) {
        const double X = P.obj[3 * i], Y = P.obj[3 * i + 1];
        const double Px = R[0] * X + R[1] * Y, Py = R[3] * X + R[4] * Y, Pz = R[6] * X + R[7] * Y;   // R X
        const double Yx = Px + t[0], Yy = Py + t[1], Yz = Pz + t[2];
        const double iz = 1.0 / Yz, a = Yx * iz, b = Yy * iz;
        const double r = std::sqrt(a * a + b * b);
        const double th = fe_atan(r);
        const double t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
        const double td = th * (1.0 + k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8);
        const double g = r == 0 ? 1.0 : td / r;
        const float* m = P.img + 2 * ((size_t)v * P.npts + i);
        res[2 * i] = fx * a * g + cx - (double)m[0];
        res[2 * i + 1] = fy * b * g + cy - (double)m[1];
        if (!Ji) continue;
        const double ir = r > 1e-12 ? 1.0 / r : 0.0;   // at the axis every derivative through r vanishes
        const double p3 = th * t2 * ir, p5 = th * t4 * ir, p7 = th * t6 * ir, p9 = th * t8 * ir;
        double* ji = Ji + 16 * (size_t)i;
        const double row[16] = {a * g, 0, 1, 0, fx * a * p3, fx * a * p5, fx * a * p7, fx * a * p9,
                                0, b * g, 0, 1, fy * b * p3, fy * b * p5, fy * b * p7, fy * b * p9};
        std::memcpy(ji, row, sizeof(row));
        const double q = 1.0 + 3 * k[0] * t2 + 5 * k[1] * t4 + 7 * k[2] * t6 + 9 * k[3] * t8;   // d theta_d / d theta
        const double gp = (q / (1.0 + r * r) - g) * ir;                                        // d g / d r
        const double mm = gp * ir;
        const double xx = g + a * a * mm, xy = a * b * mm, yy = g + b * b * mm;
        const double ux = fx * xx * iz, uy = fx * xy * iz, uz = -fx * (xx * a + xy * b) * iz;
        const double vx = fy * xy * iz, vy = fy * yy * iz, vz = -fy * (xy * a + yy * b) * iz;
        double* je = Je + 12 * (size_t)i;
        je[0] = -uy * Pz + uz * Py;
        je[1] = ux * Pz - uz * Px;
        je[2] = -ux * Py + uy * Px;
        je[3] = ux; je[4] = uy; je[5] = uz;
        je[6] = -vy * Pz + vz * Py;
        je[7] = vx * Pz - vz * Px;
        je[8] = -vx * Py + vy * Px;
        je[9] = vx; je[10] = vy; je[11] = vz;
    }
}

// residuals of one view and, when J != null, its Jacobian blocks: Ji 2 x nintr (intrinsics) and
// Je 2 x 6 (rotation step d, translation) per point
void view_terms(const Problem& P, int v, const double* in, const double* R, const double* t, double* res, double* Ji,
                double* Je)
{
    if (P.nintr == kIntrFisheye) return fisheye_terms(P, v, in, R, t, res, Ji, Je);
    const double fx = in[0], fy = in[1], cx = in[2], cy = in[3];
    const double k1 = in[4], k2 = in[5], p1 = in[6], p2 = in[7], k3 = in[8];
    for (int i = 0; i < P.npts; i++) {
        const double X = P.obj[3 * i], Y = P.obj[3 * i + 1];
        const double Px = R[0] * X + R[1] * Y, Py = R[3] * X + R[4] * Y, Pz = R[6] * X + R[7] * Y;   // R X
        const double Yx = Px + t[0], Yy = Py + t[1], Yz = Pz + t[2];
        const double iz = 1.0 / Yz, x = Yx * iz, y = Yy * iz;
        const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
        const double rad = 1 + k1 * r2 + k2 * r4 + k3 * r6;
        const double xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
        const double yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
        const float* m = P.img + 2 * ((size_t)v * P.npts + i);
        res[2 * i] = fx * xd + cx - (double)m[0];
        res[2 * i + 1] = fy * yd + cy - (double)m[1];
        if (!Ji) continue;
        double* ji = Ji + 18 * (size_t)i;
        const double a[18] = {xd, 0, 1, 0, fx * x * r2, fx * x * r4, fx * 2 * x * y, fx * (r2 + 2 * x * x), fx * x * r6,
                              0, yd, 0, 1, fy * y * r2, fy * y * r4, fy * (r2 + 2 * y * y), fy * 2 * x * y, fy * y * r6};
        std::memcpy(ji, a, sizeof(a));
        const double dr = k1 + 2 * k2 * r2 + 3 * k3 * r4;
        const double xx = rad + 2 * x * x * dr + 2 * p1 * y + 6 * p2 * x;
        const double xy = 2 * x * y * dr + 2 * p1 * x + 2 * p2 * y;
        const double yy = rad + 2 * y * y * dr + 6 * p1 * y + 2 * p2 * x;
        // d(u, v) / d(Yx, Yy, Yz)
        const double ux = fx * xx * iz, uy = fx * xy * iz, uz = -fx * (xx * x + xy * y) * iz;
        const double vx = fy * xy * iz, vy = fy * yy * iz, vz = -fy * (xy * x + yy * y) * iz;
        double* je = Je + 12 * (size_t)i;
        // d Y / d d = columns e_k x (R X): (0, -Pz, Py), (Pz, 0, -Px), (-Py, Px, 0)
        je[0] = -uy * Pz + uz * Py;
        je[1] = ux * Pz - uz * Px;
        je[2] = -ux * Py + uy * Px;
        je[3] = ux; je[4] = uy; je[5] = uz;
        je[6] = -vy * Pz + vz * Py;
        je[7] = vx * Pz - vz * Px;
        je[8] = -vx * Py + vy * Px;
        je[9] = vx; je[10] = vy; je[11] = vz;
    }
}

double total_cost(const Problem& P, const double* in, const std::vector<double>& R, const std::vector<double>& t,
                  std::vector<double>& res)
{
    double c = 0;
    for (int v = 0; v < P.nviews; v++) {
        view_terms(P, v, in, &R[9 * (size_t)v], &t[3 * (size_t)v], res.data(), nullptr, nullptr);
        for (int k = 0; k < 2 * P.npts; k++) c += res[k] * res[k];
    }
    return c;
}

// the pose of each view from its homography H (board plane -> pixels, or -> normalised
// coordinates with fx = fy = 1, cx = cy = 0): K^-1 H orthonormalised; a SLAM_* code
int poses_from_homographies(const std::vector<double>& Hs, int nviews, double fx, double fy, double cx0, double cy0,
                            std::vector<double>& R, std::vector<double>& t)
{
    const double in[2] = {fx, fy};
    for (int v = 0; v < nviews; v++) {
        const double* H = &Hs[9 * (size_t)v];
        double M[9];   // K^-1 H
        for (int k = 0; k < 3; k++) {
            M[k] = (H[k] - cx0 * H[6 + k]) / in[0];
            M[3 + k] = (H[3 + k] - cy0 * H[6 + k]) / in[1];
            M[6 + k] = H[6 + k];
        }
        const double sgn = M[8] < 0 ? -1.0 : 1.0;   // the board is in front of the camera
        double r1[3] = {M[0], M[3], M[6]}, r2[3] = {M[1], M[4], M[7]};
        const double lam = sgn / std::sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]);
        if (!std::isfinite(lam)) return SLAM_E_SOLVER;
        for (int k = 0; k < 3; k++) { r1[k] *= lam; r2[k] *= lam; t[3 * (size_t)v + k] = M[3 * k + 2] * lam; }
        // Gram-Schmidt: r1, then r2 made orthogonal to it, r3 = r1 x r2
        const double n1 = std::sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]);
        for (int k = 0; k < 3; k++) r1[k] /= n1;
        const double dt = r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2];
        for (int k = 0; k < 3; k++) r2[k] -= dt * r1[k];
        const double n2 = std::sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2]);
        if (!(n2 > 1e-12) || !std::isfinite(n2)) return SLAM_E_SOLVER;
        for (int k = 0; k < 3; k++) r2[k] /= n2;
        const double r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
        double* Rv = &R[9 * (size_t)v];
        for (int k = 0; k < 3; k++) { Rv[3 * k] = r1[k]; Rv[3 * k + 1] = r2[k]; Rv[3 * k + 2] = r3[k]; }
    }

    return SLAM_OK;
}

// Levenberg-Marquardt from (in, R, t) to the optimum; a SLAM_* code
int refine(const Problem& P, double* in, std::vector<double>& R, std::vector<double>& t, double* cost_out, int* it_out)
{
    const int nviews = P.nviews, npts = P.npts, ni = P.nintr;
    const int np = ni + 6 * nviews;
    std::vector<double> res(2 * (size_t)npts), Ji(2 * (size_t)ni * npts), Je(12 * (size_t)npts);
    std::vector<double> JtJ((size_t)np * np), g(np), A, step(np), Rn(R.size()), tn(t.size());
    double cost = total_cost(P, in, R, t, res);
    if (!std::isfinite(cost)) return SLAM_E_SOLVER;
    double lambda = 1e-3;
    int it = 0, stalled = 0;
    const int kMaxIter = 500;
    for (; it < kMaxIter && stalled < 3; it++) {
        std::fill(JtJ.begin(), JtJ.end(), 0.0);
        std::fill(g.begin(), g.end(), 0.0);
        for (int v = 0; v < nviews; v++) {
            view_terms(P, v, in, &R[9 * (size_t)v], &t[3 * (size_t)v], res.data(), Ji.data(), Je.data());
            const int e0 = ni + 6 * v;
            for (int r = 0; r < 2 * npts; r++) {
                const double* ji = &Ji[(size_t)ni * r];
                const double* je = &Je[6 * (size_t)r];
                for (int a = 0; a < ni; a++) {
                    for (int b = a; b < ni; b++) JtJ[(size_t)a * np + b] += ji[a] * ji[b];
                    for (int b = 0; b < 6; b++) JtJ[(size_t)a * np + e0 + b] += ji[a] * je[b];
                    g[a] += ji[a] * res[r];
                }
                for (int a = 0; a < 6; a++) {
                    for (int b = a; b < 6; b++) JtJ[(size_t)(e0 + a) * np + e0 + b] += je[a] * je[b];
                    g[e0 + a] += je[a] * res[r];
                }
            }
        }
        for (int a = 0; a < np; a++)
            for (int b = 0; b < a; b++) JtJ[(size_t)a * np + b] = JtJ[(size_t)b * np + a];
        bool accepted = false;
        for (int tries = 0; tries < 40 && !accepted; tries++) {
            A = JtJ;
            for (int a = 0; a < np; a++) {
                const double d = JtJ[(size_t)a * np + a];
                A[(size_t)a * np + a] = d + lambda * (d > 0 ? d : 1.0);
                step[a] = -g[a];
            }
            if (solve_dense(A, step, np)) {
                double inn[kIntr];
                for (int a = 0; a < ni; a++) inn[a] = in[a] + step[a];
                bool fine = true;
                for (int v = 0; v < nviews && fine; v++) {
                    const double* d = &step[ni + 6 * (size_t)v];
                    double E[9];
                    if (slam_rodrigues(d, 3, E) != SLAM_OK) { fine = false; break; }
                    mul33(E, &R[9 * (size_t)v], &Rn[9 * (size_t)v]);
                    for (int k = 0; k < 3; k++) tn[3 * (size_t)v + k] = t[3 * (size_t)v + k] + d[3 + k];
                }
                const double cn = fine ? total_cost(P, inn, Rn, tn, res) : INFINITY;
                if (std::isfinite(cn) && cn <= cost) {
                    // converged when accepted steps stop lowering the cost
                    stalled = (cost - cn <= 1e-15 * cost) ? stalled + 1 : 0;
                    std::memcpy(in, inn, ni * sizeof(double));
                    R.swap(Rn);
                    t.swap(tn);
                    cost = cn;
                    lambda = std::max(lambda * 0.1, 1e-12);
                    accepted = true;
                    break;
                }
            }
            lambda *= 10;
        }
        if (!accepted) break;   // no downhill step at any damping: a minimum to rounding
    }

    *cost_out = cost;
    *it_out = it;
    return SLAM_OK;
}

}  // namespace

int calibrate_camera(const float* obj, const float* img, int nviews, int npts, int size_w, int size_h, double* K,
                     double* D, double* rvecs, double* tvecs, double* rms, int* iterations)
{
    if (!obj || !img || !K || !D || !rvecs || !tvecs || !rms || !iterations) return SLAM_E_INVALID_ARG;
    if (nviews < 3 || npts < 4 || size_w <= 0 || size_h <= 0) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < npts; i++)
        if (obj[3 * i + 2] != 0.f || !std::isfinite(obj[3 * i]) || !std::isfinite(obj[3 * i + 1]))
            return SLAM_E_INVALID_ARG;            // a planar target with z = 0
    for (size_t i = 0; i < (size_t)nviews * npts * 2; i++)
        if (!std::isfinite(img[i])) return SLAM_E_INVALID_ARG;
    const Problem P{nviews, npts, obj, img, kIntr};

    // ---- initial values ----
    std::vector<double> xy(2 * (size_t)npts), uv(2 * (size_t)npts), Hs(9 * (size_t)nviews);
    for (int i = 0; i < npts; i++) { xy[2 * i] = obj[3 * i]; xy[2 * i + 1] = obj[3 * i + 1]; }
    for (int v = 0; v < nviews; v++) {
        for (int i = 0; i < 2 * npts; i++) uv[i] = img[2 * (size_t)v * npts + i];
        if (!homography(xy.data(), uv.data(), npts, &Hs[9 * (size_t)v])) return SLAM_E_SOLVER;
    }
    const double cx0 = (size_w - 1) * 0.5, cy0 = (size_h - 1) * 0.5;
    double N[3] = {0, 0, 0}, nb[2] = {0, 0};      // normal equations of the 2 nviews x 2 system in 1/fx^2, 1/fy^2
    for (int v = 0; v < nviews; v++) {
        double G[9];
        std::memcpy(G, &Hs[9 * (size_t)v], sizeof(G));
        for (int k = 0; k < 3; k++) { G[k] -= G[6 + k] * cx0; G[3 + k] -= G[6 + k] * cy0; }
        double h[3], w[3], d1[3], d2[3], n[4] = {0, 0, 0, 0};
        for (int j = 0; j < 3; j++) {
            h[j] = G[3 * j]; w[j] = G[3 * j + 1];
            d1[j] = (h[j] + w[j]) * 0.5; d2[j] = (h[j] - w[j]) * 0.5;
            n[0] += h[j] * h[j]; n[1] += w[j] * w[j]; n[2] += d1[j] * d1[j]; n[3] += d2[j] * d2[j];
        }
        for (int k = 0; k < 4; k++) n[k] = 1.0 / std::sqrt(n[k]);
        for (int j = 0; j < 3; j++) { h[j] *= n[0]; w[j] *= n[1]; d1[j] *= n[2]; d2[j] *= n[3]; }
        const double A[2][2] = {{h[0] * w[0], h[1] * w[1]}, {d1[0] * d2[0], d1[1] * d2[1]}};
        const double b[2] = {-h[2] * w[2], -d1[2] * d2[2]};
        for (int r = 0; r < 2; r++) {
            N[0] += A[r][0] * A[r][0]; N[1] += A[r][0] * A[r][1]; N[2] += A[r][1] * A[r][1];
            nb[0] += A[r][0] * b[r]; nb[1] += A[r][1] * b[r];
        }
    }
    const double det = N[0] * N[2] - N[1] * N[1];
    if (!(std::fabs(det) > 1e-14 * std::max(N[0] * N[2], DBL_MIN)) || !std::isfinite(det)) return SLAM_E_SOLVER;
    const double f0 = (N[2] * nb[0] - N[1] * nb[1]) / det, f1 = (N[0] * nb[1] - N[1] * nb[0]) / det;
    if (!(std::fabs(f0) > 0) || !(std::fabs(f1) > 0)) return SLAM_E_SOLVER;
    double in[kIntr] = {std::sqrt(std::fabs(1.0 / f0)), std::sqrt(std::fabs(1.0 / f1)), cx0, cy0, 0, 0, 0, 0, 0};
    if (!std::isfinite(in[0]) || !std::isfinite(in[1])) return SLAM_E_SOLVER;

    std::vector<double> R(9 * (size_t)nviews), t(3 * (size_t)nviews);
    if (int rc = poses_from_homographies(Hs, nviews, in[0], in[1], cx0, cy0, R, t)) return rc;

    double cost = 0;
    int it = 0;
    if (int rc = refine(P, in, R, t, &cost, &it)) return rc;

    const double k[9] = {in[0], 0, in[2], 0, in[1], in[3], 0, 0, 1};
    std::memcpy(K, k, sizeof(k));
    std::memcpy(D, in + 4, 5 * sizeof(double));
    for (int v = 0; v < nviews; v++) {
        if (slam_rodrigues(&R[9 * (size_t)v], 9, rvecs + 3 * (size_t)v) != SLAM_OK) return SLAM_E_SOLVER;
        std::memcpy(tvecs + 3 * (size_t)v, &t[3 * (size_t)v], 3 * sizeof(double));
    }
    for (int a = 0; a < kIntr; a++)
        if (!std::isfinite(in[a])) return SLAM_E_SOLVER;
    *rms = std::sqrt(cost / ((double)nviews * npts));
    *iterations = it;
    return SLAM_OK;
}

int fisheye_calibrate(const float* obj, const float* img, int nviews, int npts, int size_w, int size_h, double* K,
                      double* D, double* rvecs, double* tvecs, double* rms, int* iterations)
{
    if (!obj || !img || !K || !D || !rvecs || !tvecs || !rms || !iterations) return SLAM_E_INVALID_ARG;
    if (nviews < 3 || npts < 4 || size_w <= 0 || size_h <= 0) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < npts; i++)
        if (obj[3 * i + 2] != 0.f || !std::isfinite(obj[3 * i]) || !std::isfinite(obj[3 * i + 1]))
            return SLAM_E_INVALID_ARG;            // a planar target with z = 0
    for (size_t i = 0; i < (size_t)nviews * npts * 2; i++)
        if (!std::isfinite(img[i])) return SLAM_E_INVALID_ARG;
    const Problem P{nviews, npts, obj, img, kIntrFisheye};

    // ---- initial values: f = max(w, h) / pi, the centre, D = 0; poses from the homographies
    // board -> normalised coordinates of the points undistorted with D = 0 (theta = |pw|, below 1.5) ----
    const double f0 = std::max(size_w, size_h) / 3.14159265358979323846;
    double in[kIntr] = {f0, f0, (size_w - 1) * 0.5, (size_h - 1) * 0.5, 0, 0, 0, 0, 0};
    std::vector<double> xy(2 * (size_t)npts), uv(2 * (size_t)npts), Hs(9 * (size_t)nviews);
    for (int i = 0; i < npts; i++) { xy[2 * i] = obj[3 * i]; xy[2 * i + 1] = obj[3 * i + 1]; }
    for (int v = 0; v < nviews; v++) {
        for (int i = 0; i < npts; i++) {
            const float* m = img + 2 * ((size_t)v * npts + i);
            const double px = ((double)m[0] - in[2]) / f0, py = ((double)m[1] - in[3]) / f0;
            const double th = std::sqrt(px * px + py * py);
            const double sc = th > 1e-9 ? fe_tan(std::min(th, 1.5)) / th : 1.0;
            uv[2 * i] = px * sc;
            uv[2 * i + 1] = py * sc;
        }
        if (!homography(xy.data(), uv.data(), npts, &Hs[9 * (size_t)v])) return SLAM_E_SOLVER;
    }
    std::vector<double> R(9 * (size_t)nviews), t(3 * (size_t)nviews);
    if (int rc = poses_from_homographies(Hs, nviews, 1.0, 1.0, 0.0, 0.0, R, t)) return rc;

    double cost = 0;
    int it = 0;
    if (int rc = refine(P, in, R, t, &cost, &it)) return rc;

    const double k[9] = {in[0], 0, in[2], 0, in[1], in[3], 0, 0, 1};
    std::memcpy(K, k, sizeof(k));
    std::memcpy(D, in + 4, 4 * sizeof(double));
    for (int v = 0; v < nviews; v++) {
        if (slam_rodrigues(&R[9 * (size_t)v], 9, rvecs + 3 * (size_t)v) != SLAM_OK) return SLAM_E_SOLVER;
        std::memcpy(tvecs + 3 * (size_t)v, &t[3 * (size_t)v], 3 * sizeof(double));
    }
    for (int a = 0; a < kIntrFisheye; a++)
        if (!std::isfinite(in[a])) return SLAM_E_SOLVER;
    *rms = std::sqrt(cost / ((double)nviews * npts));
    *iterations = it;
    return SLAM_OK;
}

}  // namespace slamhip

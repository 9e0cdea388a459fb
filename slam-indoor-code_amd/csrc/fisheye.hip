// The fisheye lens model on the device: cv::fisheye of OpenCV 4.8 with the skew
// fixed at 0, restated in uncontracted f64 with the project's own arctangent
// and tangent (fisheye_math.h; DESIGN.md section 19 has the contract,
// tests/fisheye_ref.py the definition).
//
//   fisheye_map     the fixed-point map (CV_16SC2 + CV_16UC1) of
//                   fisheye::initUndistortRectifyMap with R = I and P = newK,
//                   i.e. what fisheye::undistortImage builds.  One thread walks
//                   one destination row: the row's _x, _y, _w are sequential
//                   sums by contract, as in undist_map.  No stripes.  Built once
//                   per (model, K, newK, D, w, h) into the context's map cache;
//                   undist_remap (undistort.hip) reads it unchanged.
//   fisheye_points  fisheye::undistortPoints for CV_32FC2 points without R: one
//                   thread per point runs Newton on theta, fe_tan, P and the
//                   forward model of the result for the residual.
#include "slamhip_internal.h"

#include "fisheye_math.h"

#include <cfloat>
#include <cmath>
#include <cstring>

namespace slamhip {

namespace {

struct FisheyeMapParams {
    double fx, fy, cx, cy;
    double k[4];
    double ir[9];   // the inverse of newK (K when absent), closed form
    int w, h;
};

// the forward model at normalised (a, b): distorted pixels (u, v)
__device__ __forceinline__ void fisheye_distort(double fx, double fy, double cx, double cy, const double* k, double a,
                                                double b, double& u, double& v)
{
    const double r = sqrt(a * a + b * b);
    const double theta = fe_atan(r);
    const double t2 = theta * theta;
    const double t4 = t2 * t2;
    const double t6 = t4 * t2;
    const double t8 = t4 * t4;
    const double td = theta * (1.0 + k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8);
    const double scale = r == 0 ? 1.0 : td / r;
    u = fx * a * scale + cx;
    v = fy * b * scale + cy;
}

constexpr int kMapThreads = 64;

__global__ __launch_bounds__(kMapThreads) void fisheye_map(FisheyeMapParams P, uint32_t* __restrict__ xy,
                                                           uint16_t* __restrict__ frac)
{
    const int i = blockIdx.x * kMapThreads + threadIdx.x;
    if (i >= P.h) return;
    const double* ir = P.ir;
    double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
    const size_t row = (size_t)i * P.w;
    for (int j = 0; j < P.w; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
        double u, v;
        fisheye_distort(P.fx, P.fy, P.cx, P.cy, P.k, _x / _w, _y / _w, u, v);
        const int iu = cv_round(u * 32), iv = cv_round(v * 32);
        // (short)(iu >> 5) wraps modulo 2^16, as in undist_map
        xy[row + j] = ((uint32_t)(iu >> 5) & 0xffffu) | ((uint32_t)(iv >> 5) << 16);
        frac[row + j] = (uint16_t)((iv & 31) * 32 + (iu & 31));
    }
}

constexpr int kPointThreads = 256;
constexpr double kHalfPi = 1.5707963267948966;   // CV_PI / 2
constexpr float kRejected = -1000000.f;

// One thread per point; the lanes of a wave leave the Newton loop at different
// j, and max_iter (at most kUndistMaxIter) bounds the launch.  A point is read
// before its result is written, so dst may be src itself (stride 8).
__global__ __launch_bounds__(kPointThreads) void fisheye_points(FisheyePointsParams P, const float* src, size_t src_stride,
                                                                int n, float* dst, float* err)
{
    const int i = blockIdx.x * kPointThreads + threadIdx.x;
    if (i >= n) return;
    const float* s = reinterpret_cast<const float*>(reinterpret_cast<const char*>(src) + (size_t)i * src_stride);
    const double u = s[0], v = s[1];
    const double* k = P.k;
    const double pwx = (u - P.cx) / P.fx, pwy = (v - P.cy) / P.fy;
    double td = sqrt(pwx * pwx + pwy * pwy);
    // std::min(std::max(-pi/2, td), pi/2): a NaN becomes -pi/2 (kept)
    td = -kHalfPi < td ? td : -kHalfPi;
    td = kHalfPi < td ? kHalfPi : td;
    bool converged = false;
    double theta = td, scale = 1.0;
    if (td > 1e-8) {
        for (int j = 0; j < P.max_iter; j++) {
            const double t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t6 * t2;
            const double k0 = k[0] * t2, k1 = k[1] * t4, k2 = k[2] * t6, k3 = k[3] * t8;
            const double fix = (theta * (1.0 + k0 + k1 + k2 + k3) - td) / (1.0 + 3.0 * k0 + 5.0 * k1 + 7.0 * k2 + 9.0 * k3);
            theta = theta - fix;
            if (P.use_eps && fabs(fix) < P.eps) {
                converged = true;
                break;
            }
        }
        scale = fe_tan(theta) / td;
    } else {
        converged = true;
    }
    const bool flipped = (td < 0 && theta > 0) || (td > 0 && theta < 0);
    const bool ok = (converged || !P.use_eps) && !flipped;
    const double x = pwx * scale, y = pwy * scale;
    if (err) {
        // the residual of the point that is returned (ours: OpenCV does not report it)
        double du, dv;
        fisheye_distort(P.fx, P.fy, P.cx, P.cy, k, x, y, du, dv);
        const double dx = du - u, dy = dv - v;
        err[i] = ok ? (float)sqrt(dx * dx + dy * dy) : __builtin_nanf("");
    }
    const double* RR = P.RR;
    const double xx = RR[0] * x + RR[1] * y + RR[2];
    const double yy = RR[3] * x + RR[4] * y + RR[5];
    const double ww = RR[6] * x + RR[7] * y + RR[8];
    dst[2 * (size_t)i] = ok ? (float)(xx / ww) : kRejected;
    dst[2 * (size_t)i + 1] = ok ? (float)(yy / ww) : kRejected;
}

bool finite4(const double* d)
{
    return std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]) && std::isfinite(d[3]);
}

}  // namespace

int fisheye_prepare(slam_ctx* c, hipStream_t s, int w, int h, const double* K, const double* dist, int ndist,
                    const double* newK)
{
    if (!K || !dist) return set_err(c, SLAM_E_INVALID_ARG, "fisheye undistort: null camera matrix or coefficients");
    if (w <= 0 || h <= 0) return set_err(c, SLAM_E_INVALID_ARG, "fisheye undistort: empty image");
    if (ndist != 4) return set_err(c, SLAM_E_INVALID_ARG, "fisheye undistort: exactly 4 distortion coefficients");
    if (!finite4(dist)) return set_err(c, SLAM_E_INVALID_ARG, "fisheye undistort: the coefficients are not finite");
    // sx, sy are shorts and the in-frame byte offsets (one row past the frame included) ints
    if (w > 32767 || h > 32767 || (size_t)w * (h + 2) * 3 > (size_t)INT_MAX - 16)
        return set_err(c, SLAM_E_UNSUPPORTED, "fisheye undistort: image too large");
    const double* Ar = newK ? newK : K;
    if (!(Ar[6] == 0 && Ar[7] == 0 && Ar[8] == 1))
        return set_err(c, SLAM_E_INVALID_ARG, "fisheye undistort: the last row of the new camera matrix is (0, 0, 1)");
    FisheyeMapParams P;
    std::memset(&P, 0, sizeof(P));
    if (!invert3(Ar, P.ir)) return set_err(c, SLAM_E_INVALID_ARG, "fisheye undistort: singular new camera matrix");
    P.fx = K[0];
    P.fy = K[4];
    P.cx = K[2];
    P.cy = K[5];
    std::memcpy(P.k, dist, sizeof(P.k));
    P.w = w;
    P.h = h;
    double key[30] = {};   // K, newK (K when absent), the 4 coefficients
    std::memcpy(key, K, 9 * sizeof(double));
    std::memcpy(key + 9, Ar, 9 * sizeof(double));
    std::memcpy(key + 18, dist, 4 * sizeof(double));
    return undist_cached_map(c, s, w, h, key, kLensFisheye, [&] {
        hipLaunchKernelGGL(fisheye_map, dim3((h + kMapThreads - 1) / kMapThreads), dim3(kMapThreads), 0, s, P,
                           c->undist_xy.as<uint32_t>(), c->undist_frac.as<uint16_t>());
        return hipGetLastError();
    });
}

int fisheye_points_params(slam_ctx* c, const double* K, const double* dist, int ndist, const double* P, int max_iter,
                          double eps, FisheyePointsParams* out)
{
    if (!K || !dist) return set_err(c, SLAM_E_INVALID_ARG, "fisheye undistort points: null camera matrix or coefficients");
    if (ndist != 4) return set_err(c, SLAM_E_INVALID_ARG, "fisheye undistort points: exactly 4 distortion coefficients");
    if (!finite4(dist))
        return set_err(c, SLAM_E_INVALID_ARG, "fisheye undistort points: the coefficients are not finite");
    if (max_iter < 1 || max_iter > kUndistMaxIter || !(eps >= 0) || eps > DBL_MAX)
        return set_err(c, SLAM_E_INVALID_ARG,
                       "fisheye undistort points: criteria are 1..1000 iterations and a finite eps >= 0");
    std::memset(out, 0, sizeof(*out));
    out->fx = K[0];
    out->fy = K[4];
    out->cx = K[2];
    out->cy = K[5];
    std::memcpy(out->k, dist, sizeof(out->k));
    if (P) std::memcpy(out->RR, P, sizeof(out->RR));
    else out->RR[0] = out->RR[4] = out->RR[8] = 1.;
    out->max_iter = max_iter;
    out->use_eps = eps > 0;
    out->eps = eps;
    return SLAM_OK;
}

hipError_t launch_fisheye_points(hipStream_t s, const FisheyePointsParams& P, const float* src, size_t src_stride, int n,
                                 float* dst, float* err)
{
    hipLaunchKernelGGL(fisheye_points, dim3((unsigned)(((size_t)n + kPointThreads - 1) / kPointThreads)),
                       dim3(kPointThreads), 0, s, P, src, src_stride, n, dst, err);
    return hipGetLastError();
}

}  // namespace slamhip

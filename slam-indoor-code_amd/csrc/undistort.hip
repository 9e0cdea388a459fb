// Frame undistortion on the device: cv::undistort(src, dst, K, D, newK) of
// OpenCV 4.8 restated for its scalar path with uncontracted f64 (DESIGN.md has
// the contract).  The reference leaves the seam open at batch.cpp:244 ("here
// can be undistortion"), between getNextFrame and fastExtractor.
//
//   undist_map    the fixed-point map (CV_16SC2 + CV_16UC1) of
//                 initUndistortRectifyMap, built stripe by stripe as
//                 cv::undistort does.  One thread walks one destination row:
//                 the row's _x, _y, _w are sequential sums by contract.  Runs
//                 once per (K, newK, D, w, h) and is cached in the context.
//   undist_remap  remap(INTER_LINEAR, BORDER_CONSTANT 0) of 8-bit frames, exact
//                 integer arithmetic.  A workgroup owns one destination tile and
//                 loops over a chunk of frames with the map entries and weights
//                 unpacked once; a thread produces 4 consecutive pixels.
//
// and cv::undistortPoints for the keypoints that reach geometry (the same seam,
// and the one findFirstGoodFrame marks at mainCycleInternals.cpp:142, taken the
// cheap way):
//
//   undist_points cvUndistortPointsInternal for CV_32FC2 points without R: the
//                 fixed-point iteration of the inverse model, one thread per
//                 point in uncontracted f64, with the reprojection residual of
//                 the returned point as a second output.
#include "slamhip_internal.h"

#include <cfloat>
#include <climits>
#include <cstring>

namespace slamhip {

namespace {

struct UndistParams {
    double A[9];    // K
    double Ar[9];   // newK (K when absent)
    double D[12];   // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4
    int w, h, stripe;
};

constexpr int kMapThreads = 64;

__global__ __launch_bounds__(kMapThreads) void undist_map(UndistParams P, uint32_t* __restrict__ xy,
                                                          uint16_t* __restrict__ frac)
{
    const int r = blockIdx.x * kMapThreads + threadIdx.x;
    if (r >= P.h) return;
    const int i = r % P.stripe, y0 = r - i;
    double a[9], ir[9];
    for (int k = 0; k < 9; k++) a[k] = P.Ar[k];
    a[5] = P.Ar[5] - (double)y0;
    if (!invert3(a, ir)) return;   // the host has checked every stripe
    const double fx = P.A[0], fy = P.A[4], u0 = P.A[2], v0 = P.A[5];
    const double k1 = P.D[0], k2 = P.D[1], p1 = P.D[2], p2 = P.D[3], k3 = P.D[4], k4 = P.D[5], k5 = P.D[6],
                 k6 = P.D[7], s1 = P.D[8], s2 = P.D[9], s3 = P.D[10], s4 = P.D[11];
    double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
    const size_t row = (size_t)r * P.w;
    for (int j = 0; j < P.w; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
        const double w = 1. / _w, x = _x * w, y = _y * w;
        const double x2 = x * x, y2 = y * y;
        const double r2 = x2 + y2, _2xy = 2 * x * y;
        const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
        const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2;
        const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2;
        const double u = fx * xd + u0;
        const double v = fy * yd + v0;
        const int iu = cv_round(u * 32), iv = cv_round(v * 32);
        // (short)(iu >> 5): the cast wraps modulo 2^16 (kept)
        xy[row + j] = ((uint32_t)(iu >> 5) & 0xffffu) | ((uint32_t)(iv >> 5) << 16);
        frac[row + j] = (uint16_t)((iv & 31) * 32 + (iu & 31));
    }
}

// ---- remap ---------------------------------------------------------------------

// 32 threads x 4 pixels across, 8 rows: 256 threads per destination tile
constexpr int kPx = 4;
constexpr int kThreadsX = kUndistTileW / kPx;
constexpr int kRemapThreads = kThreadsX * kUndistTileH;

// The source is read as aligned dwords of the whole batch: a dword with at
// least one byte of the batch in it lies in the batch's pages.  Within a frame
// dwords are indexed from the one holding the frame's first byte (a 32-bit
// index, negative for the row above the frame) and clamped to the batch's
// first and last dword as seen from that frame; a clamped load only ever feeds
// a tap whose weight is 0.
struct SrcWords {
    const uint32_t* frame;   // the dword holding the frame's first byte
    int lo, hi;              // the batch's first and last dword, relative to it
    __device__ __forceinline__ uint32_t at(int i) const { return frame[min(max(i, lo), hi)]; }
};

// CH bytes of each of two horizontally adjacent pixels, starting at byte p of
// S.frame (p >= -(row + CH) - 3: a tap of a partly valid pixel, plus the frame's misalignment)
template <int CH>
__device__ __forceinline__ void load_pair(const SrcWords& S, int p, int (&s0)[CH], int (&s1)[CH])
{
    const int d = p >> 2;
    const unsigned sh = (unsigned)p & 3u;
    const uint32_t q0 = S.at(d), q1 = S.at(d + 1);
    const uint32_t lo = __builtin_amdgcn_alignbyte(q1, q0, sh);   // bytes p .. p + 3
    if constexpr (CH == 1) {
        s0[0] = lo & 255u;
        s1[0] = (lo >> 8) & 255u;
    } else {
        const uint32_t q2 = S.at(d + 2);
        const uint32_t hi = __builtin_amdgcn_alignbyte(q2, q1, sh);   // bytes p + 4 .. p + 7
        s0[0] = lo & 255u;
        s0[1] = (lo >> 8) & 255u;
        s0[2] = (lo >> 16) & 255u;
        s1[0] = lo >> 24;
        s1[1] = hi & 255u;
        s1[2] = (hi >> 8) & 255u;
    }
}

template <int CH>
__global__ __launch_bounds__(kRemapThreads) void undist_remap(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              const uint32_t* __restrict__ xy,
                                                              const uint16_t* __restrict__ frac, int nframes, int w,
                                                              int h)
{
    const int tx = threadIdx.x % kThreadsX, ty = threadIdx.x / kThreadsX;
    const int x0 = blockIdx.x * kUndistTileW + tx * kPx;
    const int y = blockIdx.y * kUndistTileH + ty;
    if (y >= h || x0 >= w) return;
    const int npx = min(kPx, w - x0);
    const int row = w * CH;
    const size_t fb = (size_t)row * h;

    // the map entries of this thread's pixels, unpacked once for all frames:
    // the byte offset of tap 00 in its frame and the four weights, zero where
    // the tap lies outside the source (BORDER_CONSTANT 0)
    int off[kPx], w00[kPx], w01[kPx], w10[kPx], w11[kPx];
#pragma unroll
    for (int k = 0; k < kPx; k++) {
        off[k] = 0;
        w00[k] = w01[k] = w10[k] = w11[k] = 0;
        if (k < npx) {
            const size_t m = (size_t)y * w + x0 + k;
            const uint32_t e = xy[m];
            const int sx = (int16_t)(e & 0xffffu), sy = (int16_t)(e >> 16);
            const int fr = frac[m];
            const int a = fr & 31, b = fr >> 5;
            const bool cx0 = sx >= 0 && sx < w, cx1 = sx + 1 >= 0 && sx + 1 < w;
            const bool cy0 = sy >= 0 && sy < h, cy1 = sy + 1 >= 0 && sy + 1 < h;
            if ((cx0 || cx1) && (cy0 || cy1)) {
                off[k] = sy * row + sx * CH;
                w00[k] = cx0 && cy0 ? (32 - b) * (32 - a) * 32 : 0;
                w01[k] = cx1 && cy0 ? (32 - b) * a * 32 : 0;
                w10[k] = cx0 && cy1 ? b * (32 - a) * 32 : 0;
                w11[k] = cx1 && cy1 ? b * a * 32 : 0;
            }
        }
    }

    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(src) & 3u);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(src - mis);   // d_src rounded down to a dword
    const long long last = (long long)((mis + fb * (size_t)nframes - 1) >> 2);   // the dword of the batch's last byte
    const int f0 = blockIdx.z * kUndistFrames;
    const int f1 = min(nframes, f0 + kUndistFrames);
    const size_t dpix = (size_t)y * row + (size_t)x0 * CH;

    for (int f = f0; f < f1; f++) {
        const size_t fbyte = mis + fb * (size_t)f;       // the frame's first byte, from `words`
        const long long fword = (long long)(fbyte >> 2);
        const int fmis = (int)(fbyte & 3u);
        SrcWords S;
        S.frame = words + fword;
        S.lo = (int)max(-fword, (long long)INT_MIN);
        S.hi = (int)min(last - fword, (long long)INT_MAX);
        uint8_t o[kPx * CH];
#pragma unroll
        for (int k = 0; k < kPx; k++) {
            int a0[CH], a1[CH], b0[CH], b1[CH];
            const int p = fmis + off[k];
            load_pair<CH>(S, p, a0, a1);
            load_pair<CH>(S, p + row, b0, b1);
#pragma unroll
            for (int c = 0; c < CH; c++)
                o[k * CH + c] = (uint8_t)((a0[c] * w00[k] + a1[c] * w01[k] + b0[c] * w10[k] + b1[c] * w11[k] + 16384) >> 15);
        }
        uint8_t* d = dst + fb * (size_t)f + dpix;
        if (npx == kPx && (reinterpret_cast<uintptr_t>(d) & 3u) == 0) {
            uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
#pragma unroll
            for (int q = 0; q < CH; q++)
                d4[q] = (uint32_t)o[4 * q] | ((uint32_t)o[4 * q + 1] << 8) | ((uint32_t)o[4 * q + 2] << 16) |
                        ((uint32_t)o[4 * q + 3] << 24);
        } else {
            // a row or frame start that is not dword-aligned, or the row's tail: by the byte
#pragma unroll
            for (int k = 0; k < kPx; k++)
                if (k < npx) {
#pragma unroll
                    for (int c = 0; c < CH; c++) d[k * CH + c] = o[k * CH + c];
                }
        }
    }
}

// ---- undistortPoints -------------------------------------------------------------

// the forward model at (x, y) and its pixel distance to the input point (u, v):
// the EPS block of cvUndistortPointsInternal, operation by operation
__device__ __forceinline__ double undist_reproject(const UndistPointsParams& P, double x, double y, double u, double v)
{
    const double* k = P.k;
    const double r2 = x * x + y * y;
    const double r4 = r2 * r2;
    const double r6 = r4 * r2;
    const double a1 = 2 * x * y;
    const double a2 = r2 + 2 * x * x;
    const double a3 = r2 + 2 * y * y;
    const double cdist = 1 + k[0] * r2 + k[1] * r4 + k[4] * r6;
    const double icdist2 = 1. / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6);
    const double xd = x * cdist * icdist2 + k[2] * a1 + k[3] * a2 + k[8] * r2 + k[9] * r4;
    const double yd = y * cdist * icdist2 + k[2] * a3 + k[3] * a1 + k[10] * r2 + k[11] * r4;
    const double dx = xd * P.fx + P.cx - u;
    const double dy = yd * P.fy + P.cy - v;
    return sqrt(dx * dx + dy * dy);
}

constexpr int kPointThreads = 256;

// One thread per point.  The lanes of a wave leave the loop at different j;
// max_iter (at most kUndistMaxIter) bounds the launch.  A point is read before
// its result is written, so dst may be src itself (stride 8).
__global__ __launch_bounds__(kPointThreads) void undist_points(UndistPointsParams P, const float* src, size_t src_stride,
                                                               int n, float* dst, float* err)
{
    const int i = blockIdx.x * kPointThreads + threadIdx.x;
    if (i >= n) return;
    const float* s = reinterpret_cast<const float*>(reinterpret_cast<const char*>(src) + (size_t)i * src_stride);
    const double u = s[0], v = s[1];
    const double* k = P.k;
    double x = (u - P.cx) * P.ifx, y = (v - P.cy) * P.ify;
    const double x0 = x, y0 = y;
    double error = DBL_MAX;
    for (int j = 0;; j++) {
        if (j >= P.max_iter) break;
        if (P.use_eps && error < P.eps) break;
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        if (icdist < 0) {   // OpenCV's test of regression 14583: back to the start value (kept)
            x = (u - P.cx) * P.ifx;
            y = (v - P.cy) * P.ify;
            break;
        }
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
        if (P.use_eps) error = undist_reproject(P, x, y, u, v);
    }
    // the residual of the point that is returned (ours: OpenCV does not report it)
    if (err) err[i] = (float)undist_reproject(P, x, y, u, v);
    const double* RR = P.RR;
    const double xx = RR[0] * x + RR[1] * y + RR[2];
    const double yy = RR[3] * x + RR[4] * y + RR[5];
    const double ww = 1. / (RR[6] * x + RR[7] * y + RR[8]);
    dst[2 * (size_t)i] = (float)(xx * ww);
    dst[2 * (size_t)i + 1] = (float)(yy * ww);
}

hipError_t build_map(slam_ctx* c, hipStream_t s, const UndistParams& P)
{
    hipLaunchKernelGGL(undist_map, dim3((P.h + kMapThreads - 1) / kMapThreads), dim3(kMapThreads), 0, s, P,
                       c->undist_xy.as<uint32_t>(), c->undist_frac.as<uint16_t>());
    return hipGetLastError();
}

}  // namespace

int undist_prepare(slam_ctx* c, hipStream_t s, int w, int h, const double* K, const double* dist, int ndist,
                   const double* newK)
{
    if (!K || (ndist > 0 && !dist)) return set_err(c, SLAM_E_INVALID_ARG, "undistort: null camera matrix or coefficients");
    if (w <= 0 || h <= 0) return set_err(c, SLAM_E_INVALID_ARG, "undistort: empty image");
    if (ndist == 14) return set_err(c, SLAM_E_UNSUPPORTED, "undistort: the 14-coefficient tilt model is not supported");
    if (ndist != 4 && ndist != 5 && ndist != 8 && ndist != 12)
        return set_err(c, SLAM_E_INVALID_ARG, "undistort: 4, 5, 8 or 12 distortion coefficients");
    // sx, sy are shorts and the in-frame byte offsets (one row past the frame included) ints
    if (w > 32767 || h > 32767 || (size_t)w * (h + 2) * 3 > (size_t)INT_MAX - 16)
        return set_err(c, SLAM_E_UNSUPPORTED, "undistort: image too large");
    UndistParams P;
    std::memset(&P, 0, sizeof(P));
    std::memcpy(P.A, K, sizeof(P.A));
    std::memcpy(P.Ar, newK ? newK : K, sizeof(P.Ar));
    std::memcpy(P.D, dist, sizeof(double) * ndist);
    P.w = w;
    P.h = h;
    P.stripe = std::min(std::max(1, 4096 / std::max(w, 1)), h);
    for (int y0 = 0; y0 < h; y0 += P.stripe) {
        double a[9], ir[9];
        std::memcpy(a, P.Ar, sizeof(a));
        a[5] = P.Ar[5] - (double)y0;
        if (!invert3(a, ir)) return set_err(c, SLAM_E_INVALID_ARG, "undistort: singular new camera matrix");
    }
    static_assert(sizeof(P.A) + sizeof(P.Ar) + sizeof(P.D) == sizeof(c->undist_key), "cache key layout");
    double key[30];
    std::memcpy(key, P.A, sizeof(key));
    return undist_cached_map(c, s, w, h, key, kLensBrown, [&] { return build_map(c, s, P); });
}

int undist_cached_map(slam_ctx* c, hipStream_t s, int w, int h, const double (&key)[30], int model,
                      const std::function<hipError_t()>& build)
{
    const bool hit = c->undist_valid && c->undist_model == model && c->undist_w == w && c->undist_h == h &&
                     std::memcmp(c->undist_key, key, sizeof(c->undist_key)) == 0;
    if (!c->undist_ev) SLAM_HIP(c, hipEventCreateWithFlags(&c->undist_ev, hipEventDisableTiming));
    if (!hit) {
        c->undist_valid = false;
        // a remap queued on another stream may still read the old map
        if (c->undist_used && c->undist_stream != s) SLAM_HIP(c, hipStreamWaitEvent(s, c->undist_ev, 0));
        SLAM_HIP(c, c->undist_xy.ensure((size_t)w * h * sizeof(uint32_t)));
        SLAM_HIP(c, c->undist_frac.ensure((size_t)w * h * sizeof(uint16_t)));
        SLAM_HIP(c, build());
        std::memcpy(c->undist_key, key, sizeof(c->undist_key));
        c->undist_model = model;
        c->undist_w = w;
        c->undist_h = h;
        c->undist_valid = true;
    } else if (c->undist_stream != s) {
        SLAM_HIP(c, hipStreamWaitEvent(s, c->undist_ev, 0));   // built, or last read, on another stream
    }
    c->undist_used = true;
    c->undist_stream = s;
    SLAM_HIP(c, hipEventRecord(c->undist_ev, s));
    return SLAM_OK;
}

// the last use of the map on s is over from here (for the next caller on another stream)
int undist_mark(slam_ctx* c, hipStream_t s)
{
    SLAM_HIP(c, hipEventRecord(c->undist_ev, s));
    return SLAM_OK;
}

hipError_t launch_undist_remap(slam_ctx* c, hipStream_t s, const uint8_t* src, uint8_t* dst, int nframes, int w, int h,
                               int channels)
{
    const dim3 grid((w + kUndistTileW - 1) / kUndistTileW, (h + kUndistTileH - 1) / kUndistTileH,
                    (nframes + kUndistFrames - 1) / kUndistFrames);
    const uint32_t* xy = c->undist_xy.as<uint32_t>();
    const uint16_t* fr = c->undist_frac.as<uint16_t>();
    if (channels == 1)
        hipLaunchKernelGGL(undist_remap<1>, grid, dim3(kRemapThreads), 0, s, src, dst, xy, fr, nframes, w, h);
    else
        hipLaunchKernelGGL(undist_remap<3>, grid, dim3(kRemapThreads), 0, s, src, dst, xy, fr, nframes, w, h);
    return hipGetLastError();
}

int undist_points_params(slam_ctx* c, const double* K, const double* dist, int ndist, const double* P, int max_iter,
                         double eps, UndistPointsParams* out)
{
    if (!K || (ndist > 0 && !dist))
        return set_err(c, SLAM_E_INVALID_ARG, "undistort points: null camera matrix or coefficients");
    if (ndist == 14)
        return set_err(c, SLAM_E_UNSUPPORTED, "undistort points: the 14-coefficient tilt model is not supported");
    if (ndist != 4 && ndist != 5 && ndist != 8 && ndist != 12)
        return set_err(c, SLAM_E_INVALID_ARG, "undistort points: 4, 5, 8 or 12 distortion coefficients");
    // a count is required: OpenCV's EPS-only loop never ends on a point that does not converge
    if (max_iter < 1 || max_iter > kUndistMaxIter || !(eps >= 0) || eps > DBL_MAX)
        return set_err(c, SLAM_E_INVALID_ARG, "undistort points: criteria are 1..1000 iterations and a finite eps >= 0");
    std::memset(out, 0, sizeof(*out));
    out->fx = K[0];
    out->fy = K[4];
    out->cx = K[2];
    out->cy = K[5];
    out->ifx = 1. / K[0];
    out->ify = 1. / K[4];
    std::memcpy(out->k, dist, sizeof(double) * ndist);
    if (P) std::memcpy(out->RR, P, sizeof(out->RR));
    else out->RR[0] = out->RR[4] = out->RR[8] = 1.;
    out->max_iter = max_iter;
    out->use_eps = eps > 0;
    out->eps = eps;
    return SLAM_OK;
}

hipError_t launch_undist_points(hipStream_t s, const UndistPointsParams& P, const float* src, size_t src_stride, int n,
                                float* dst, float* err)
{
    hipLaunchKernelGGL(undist_points, dim3((unsigned)(((size_t)n + kPointThreads - 1) / kPointThreads)), dim3(kPointThreads), 0, s,
                       P, src,
                       src_stride, n, dst, err);
    return hipGetLastError();
}

}  // namespace slamhip
